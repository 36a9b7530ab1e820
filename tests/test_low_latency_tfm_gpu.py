"""The low-latency plan of the transformer trunks (P3HIP_FLAG_LOW_LATENCY_TFM: csrc/transformer_split.hip, a block's
launches split across more workgroups) on the HIP engine, through the C ABI.  The plan computes every query row and every
token row as the default fp16 plan does, so the check is an equality: a flagged engine against a default engine on the
same weights and positions, byte for byte: the 1889 raw floats of every slot, and the residual stream x and q, k, v, o
(with their padding rows, which stay zero) after a pass stopped in front of block 1 and behind the last block; for every
split of the kernels' sets forced with P3HIP_TFM_SPLIT and for the chooser's own, at batches 1, 2 (2 x 361 tokens: the
16-token tile 22 spans both positions and the last tile holds 2 tokens) and 7 (2527 tokens end every tile size mid-tile).
Then what composes with it: partial runs, launch-graph replay, AUX, symmetry averaging, the NN cache, score and loss,
the timing hook, and an evaluation match whose candidate is a transformer with nn_low_latency: 1."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ALL_SPLITS = [(s, t) for s in (1, 2, 3, 6) for t in (16, 32, 64)]
# D = 32 with x1 in LDS, D = 64 with x1 in registers: every split; D = 32 at d = 64 and D = 64 at d = 384 (V = 80, the
# largest LDS): the three splits the chooser takes below 43 positions; the other stream widths and head counts (d = 192,
# 256 and 384 with 12 heads): both token-tile counts of the split kernels
JOBS = [(n, st) for n in ("test_b2d96h3_tfm", "test_b2d128h2_tfm") for st in ALL_SPLITS] + \
       [(n, st) for n in ("test_b2d64h2_tfm", "test_b2d384h6_tfm") for st in ((6, 16), (3, 32), (2, 64))] + \
       [(n, st) for n in ("test_b2d192h6_tfm", "test_b2d256h4_tfm", "test_b2d384h12_tfm") for st in ((6, 16), (3, 32))]
NETS = ["test_b2d96h3_tfm", "test_b2d128h2_tfm", "test_b2d64h2_tfm", "test_b2d384h6_tfm"]
BATCHES = (1, 2, 7)
COMPOSE_NET = "test_b2d96h3_tfm"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> .p3w of netspec.generate_weights(cfg, randomize=True), written on demand"""
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("low_latency_tfm")
    cache = {}

    def get(name):
        if name not in cache:
            cfg = netspec.get_config(name)
            cache[name] = os.path.join(d, name + ".p3w")
            netspec.save_p3w(cache[name], cfg, netspec.generate_weights(cfg, randomize=True))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def positions():
    from p3achygo_amd import features
    return features.random_positions(16, seed=43, n_games=16, max_moves=300, komis=(7.5, -7.5, 0.5))


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    monkeypatch.delenv("P3HIP_TFM_SPLIT", raising=False)
    monkeypatch.delenv("P3HIP_DEBUG_STOP_BLOCK", raising=False)
    return monkeypatch


def _flag():
    from p3achygo_amd import engine
    return engine.FLAG_LOW_LATENCY_TFM


def _snapshot(path, name, pos, flags, env):
    """every tensor the comparison covers, as bytes: the raw outputs of a whole pass, and x, q, k, v, o of passes stopped
    in front of block 1 and behind the last block (P3HIP_DEBUG_STOP_BLOCK is read at create)"""
    from p3achygo_amd import engine, netspec
    cfg = netspec.get_config(name)
    d, heads, nblk = cfg.channels, cfg.bottleneck_channels, cfg.blocks
    Cs = 128 if d <= 128 else (256 if d <= 256 else 384)
    n = len(pos)
    out = {}
    for stop in (None, 1, nblk):
        if stop is None:
            env.delenv("P3HIP_DEBUG_STOP_BLOCK", raising=False)
        else:
            env.setenv("P3HIP_DEBUG_STOP_BLOCK", str(stop))
        eng = engine.HipEngine(path, n, flags=flags)
        eng.load_all(pos)
        eng.RunInference()
        if stop is None:
            out["raw"] = np.stack([eng.get_raw(s) for s in range(n)])
        else:
            out["x%d" % stop] = eng.debug_x(n, Cs)
            for w, t in enumerate("qkvo"):
                out["%s%d" % (t, stop)] = eng.debug_tfm(w, n, heads, d // heads)
        eng.close()
    env.delenv("P3HIP_DEBUG_STOP_BLOCK", raising=False)
    return out


_REFERENCE = {}


def _reference(files, positions, name, batch, env):
    """the default engine's snapshot, computed once per (net, batch) and never changed"""
    key = (name, batch)
    if key not in _REFERENCE:
        env.delenv("P3HIP_TFM_SPLIT", raising=False)
        ref = _snapshot(files(name), name, positions[:batch], 0, env)
        assert ref["raw"].shape == (batch, 1889) and np.isfinite(ref["raw"]).all() and np.abs(ref["raw"]).max() > 0
        for k, a in ref.items():
            assert np.isfinite(a).all() and np.abs(a).max() > 0, (name, batch, k)
            if k[0] in "qkv":
                assert (a[:, :, 361:] == 0).all(), (name, batch, k)   # the padding rows
            a.setflags(write=False)
        _REFERENCE[key] = ref
    return _REFERENCE[key]


def _compare(files, positions, name, env, label):
    for batch in BATCHES:
        want = _reference(files, positions, name, batch, env)
        if label != "chooser":
            env.setenv("P3HIP_TFM_SPLIT", label)
        got = _snapshot(files(name), name, positions[:batch], _flag(), env)
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), \
                (name, label, batch, k, np.argwhere(got[k] != want[k])[:5])
            if k[0] in "qkv":
                assert (got[k][:, :, 361:] == 0).all(), (name, label, batch, k)


@pytest.mark.parametrize("name,split", JOBS, ids=["%s-%d,%d" % (n, s, t) for n, (s, t) in JOBS])
def test_forced_split_gives_the_default_plans_bytes(built, files, positions, _clean_env, name, split):
    from p3achygo_amd import engine
    assert engine.debug_plan(files(name), _flag())[0] == "TfmSplit" and engine.debug_plan(files(name), 0)[0] == "Tfm"
    _compare(files, positions, name, _clean_env, "%d,%d" % split)


@pytest.mark.parametrize("name", NETS)
def test_chosen_split_gives_the_default_plans_bytes(built, files, positions, _clean_env, name):
    from p3achygo_amd import engine, netspec
    heads = netspec.get_config(name).bottleneck_channels
    assert all(engine.debug_tfm_split(b, heads) == (6, 16) for b in BATCHES)   # on 256 CUs; whatever it is, the bytes hold
    _compare(files, positions, name, _clean_env, "chooser")


def _pair(files, batch, extra=0):
    from p3achygo_amd import engine
    return (engine.HipEngine(files(COMPOSE_NET), batch, flags=extra),
            engine.HipEngine(files(COMPOSE_NET), batch, flags=_flag() | extra))


def test_partial_run_returns_the_default_engines_bytes(built, files, positions):
    """a batch-8 engine with slots 1, 4 and 6 loaded: a compacted pass over 3 positions"""
    raws = []
    for eng in _pair(files, 8):
        for s in (1, 4, 6):
            eng.LoadBatch(s, positions[s:s + 1])
        eng.RunInference()
        raws.append(np.stack([eng.get_raw(s) for s in (1, 4, 6)]))
        eng.close()
    assert np.abs(raws[0]).max() > 0 and raws[0].tobytes() == raws[1].tobytes()


def test_launch_graph_replays_the_default_engines_bytes(built, files, positions):
    from p3achygo_amd import engine
    B = 5
    ref = engine.HipEngine(files(COMPOSE_NET), B)
    ref.load_all(positions[:B])
    ref.RunInference()
    want = np.stack([ref.get_raw(s) for s in range(B)])
    ref.close()
    gr = engine.HipEngine(files(COMPOSE_NET), B, flags=_flag() | engine.FLAG_LAUNCH_GRAPH)
    for rnd in range(3):                       # eager, capture, replay
        gr.load_all(positions[:B])
        gr.RunInference()
        got = np.stack([gr.get_raw(s) for s in range(B)])
        assert got.tobytes() == want.tobytes(), rnd
        assert gr.graph_state() == (1 if rnd >= 1 else 0)
    gr.close()


def test_aux_record_is_the_default_engines(built, files, positions):
    from p3achygo_amd import engine
    recs = []
    for eng in _pair(files, 4, engine.FLAG_AUX):
        eng.load_all(positions[:4])
        eng.RunInference()
        recs.append(np.stack([np.concatenate([eng.GetAux(s), eng.get_raw(s)]) for s in range(4)]))
        eng.close()
    assert recs[0].shape == (4, 837 + 1889) and np.abs(recs[0][:, :837]).max() > 0
    assert recs[0].tobytes() == recs[1].tobytes()


def test_symmetry_averaged_rows_are_the_default_engines(built, files, positions):
    from p3achygo_amd import engine
    rows = []
    for eng in _pair(files, 3, engine.FLAG_SYMMETRY_AVG):
        eng.set_symmetries(0b00100101)
        eng.load_all(positions[:3])
        eng.RunInference()
        rows.append(np.stack([eng.get_raw(s) for s in range(3)]))
        eng.close()
    assert np.abs(rows[0]).max() > 0 and rows[0].tobytes() == rows[1].tobytes()


def test_nn_cache_hits_are_the_default_engines_bytes(built, files, positions):
    key = lambda i: (0x9E3779B97F4A7C15 * (i + 1) & (2**64 - 1), 0xC2B2AE3D27D4EB4F * (i + 7) & (2**64 - 1))
    outs = []
    for eng in _pair(files, 6):
        eng.EnableCache(8)
        for s in range(6):
            eng.LoadBatchKeyed(s, positions[s:s + 1], *key(s), symmetry=s % 8)
        eng.RunInference()
        first = np.stack([eng.get_raw(s) for s in range(6)])
        for s in range(6):   # three hits and three new positions: a pass over the misses alone
            k = 5 - s if s < 3 else s + 6
            eng.LoadBatchKeyed(s, positions[k:k + 1], *key(k), symmetry=1)
        eng.RunInference()
        hits = [eng.GetBatchKeyed(s)[2] for s in range(6)]
        assert hits == [True] * 3 + [False] * 3
        outs.append(np.concatenate([first, np.stack([eng.get_raw(s) for s in range(6)])]))
        eng.close()
    assert outs[0].tobytes() == outs[1].tobytes()
    assert np.array_equal(outs[0][6:9], outs[0][5:2:-1])


def test_score_and_loss_are_the_default_engines(built, files, positions):
    from p3achygo_amd import engine
    rng = np.random.default_rng(5)
    labels = np.zeros(4, engine.labels_dtype())
    targets = np.zeros(4, engine.targets_dtype())
    for s in range(4):
        mv = int(rng.integers(0, 362))
        labels[s]["policy"][mv] = 1.0
        labels[s]["score_margin"] = float(rng.integers(-30, 30)) + 0.5
        labels[s]["did_win"] = s & 1
        targets[s]["policy"][mv] = 1.0
        targets[s]["own"] = rng.integers(-1, 2, 361)
        targets[s]["score_margin"] = labels[s]["score_margin"]
        targets[s]["q6"], targets[s]["q16"], targets[s]["q50"] = rng.uniform(-1, 1, 3)
    outs = []
    for eng in _pair(files, 4, engine.FLAG_AUX):
        eng.load_all(positions[:4])
        for s in range(4):
            eng.load_labels(s, labels[s:s + 1])
            eng.load_targets(s, targets[s:s + 1])
        eng.RunInference()
        sums, n = eng.score()
        lsums, ln = eng.loss()
        assert n == 4 and ln == 4
        outs.append(np.concatenate([sums, lsums] + [eng.get_score(s).astype(np.float64) for s in range(4)] +
                                   [eng.get_loss(s).astype(np.float64) for s in range(4)]))
        eng.close()
    assert outs[0].tobytes() == outs[1].tobytes()


def test_timing_hook_names_the_attention_launch_of_the_split(built, files, positions, _clean_env):
    from p3achygo_amd import engine
    flops = 2.0 * 1 * 2.0 * 361 * 361 * 96
    for override, want in ((None, "k_tfm_attn_split"), ("1,64", "k_tfm_attn"), ("2,64", "k_tfm_attn_split")):
        if override:
            _clean_env.setenv("P3HIP_TFM_SPLIT", override)
        eng = engine.HipEngine(files(COMPOSE_NET), 1, flags=_flag())
        eng.load_all(positions[:1])
        eng.upload()
        ms, fl, kname = eng.time_trunk_kernel(1, 3)
        eng.close()
        assert ms > 0 and kname == want and fl == flops, (override, ms, kname, fl)
    _clean_env.delenv("P3HIP_TFM_SPLIT", raising=False)
    eng = engine.HipEngine(files(COMPOSE_NET), 1)
    eng.load_all(positions[:1])
    eng.upload()
    assert eng.time_trunk_kernel(1, 3)[1:] == (flops, "k_tfm_attn")
    eng.close()


def test_eval_match_with_a_low_latency_transformer_player(built, files):
    """nn_low_latency: 1 is P3HIP_FLAG_LOW_LATENCY_ANY: a candidate with a transformer net is served (P3HIP_FLAG_LOW_LATENCY
    alone fails its create), beside a current player on the default plan"""
    from p3achygo_amd import host_api
    w = files(COMPOSE_NET)
    try:
        host_api.eval_set_player_flags(cur="n: 16\n", cand="n: 16\nnn_low_latency: 1\n")
        st = host_api.eval_match(w, w, num_games=2, visits_per_move=16, leaves_per_round=4, max_moves=24, num_threads=2, seed=2)
    finally:
        host_api.eval_set_player_flags()
    assert st.games == 2 and st.cur_wins + st.cand_wins + st.draws == 2
