"""A symmetry set per slot on the MI355X (P3HIP_FLAG_SYMMETRY_SLOT).

Everything is bit for bit against a plain engine run over the copies the CPU-pinned numpy expand makes
(tests/symavg_restatement.py), its rows un-rotated and averaged in numpy float32 in the stated order, taken per slot
with that slot's own mask: the forward pass of a row does not depend on the other rows of its batch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import symavg_restatement as sr  # noqa: E402

pytestmark = pytest.mark.gpu

CYCLE = (0xFF, 0x01, 0x10, 0x81, 0x02, 0x7E, 0x80)


def _cycle(n):
    return [CYCLE[i % len(CYCLE)] for i in range(n)]


@pytest.fixture(scope="module")
def fwd(built):
    from p3achygo_amd import engine
    return engine.symmetry_maps()[0]


def _rows(eng, slots):
    rows, owns = [], []
    for s in slots:
        raw = eng.get_raw(s)
        owns.append(eng.GetOwnership(s))
        rows.append(sr.row_of(eng.GetBatch(s), raw))
    return np.stack(rows), np.stack(owns)


def _copies(pos, masks, fwd):
    """the copies of all positions, each under its own mask, packed densely in slot order"""
    return np.concatenate([sr.expand(pos[i:i + 1], m, fwd) for i, m in enumerate(masks)])


def _restated(plain, pos, masks, fwd):
    """per slot: the plain engine's rows of its copies, un-rotated and averaged with that slot's mask"""
    cp = _copies(pos, masks, fwd)
    assert len(cp) <= plain.batch_size
    for i in range(len(cp)):
        plain.LoadBatch(i, cp[i:i + 1])
    plain.RunInference()
    rows, _ = _rows(plain, range(len(cp)))
    out, at = [], 0
    for m in masks:
        k = len(sr.syms_of(m))
        out.append(sr.reduce(list(rows[at:at + k]), m, fwd))
        at += k
    return np.stack(out)


def _load(eng, pos, masks, slots=None):
    slots = range(len(pos)) if slots is None else slots
    for i, s in enumerate(slots):
        eng.LoadBatch(s, pos[i:i + 1])
        eng.set_slot_symmetries(s, masks[i])


def _evaluate(eng, pos, masks):
    _load(eng, pos, masks)
    eng.RunInference()
    return _rows(eng, range(len(pos)))


def _check_rule(path, pos, fwd, flags=0, scales=None):
    from p3achygo_amd import engine
    n = len(pos)
    masks = _cycle(n)
    assert masks[0] == 0xFF and bin(masks[-1]).count("1") == 1
    plain = engine.HipEngine(path, 8 * n, flags=flags)
    eng = engine.HipEngine(path, n, flags=flags | engine.FLAG_SYMMETRY_SLOT)
    try:
        if scales is not None:
            plain.set_int8_scales(scales)
            eng.set_int8_scales(scales)
        got, own = _evaluate(eng, pos, masks)
        want = _restated(plain, pos, masks, fwd)
        assert got.tobytes() == want.tobytes(), np.argwhere(got != want)[:5]
        assert own.tobytes() == got[:, sr.OWNERSHIP].tobytes()
    finally:
        eng.close()
        plain.close()


def test_rule_bit_for_bit(built, weight_files, fwd):
    from p3achygo_amd import features
    _check_rule(weight_files("test_b3c256btl1"), features.random_positions(37, seed=61), fwd)


def test_rule_bit_for_bit_c384(built, weight_files, fwd):
    from p3achygo_amd import features
    _check_rule(weight_files("test_b3c384btl3"), features.random_positions(37, seed=62), fwd)


def _tfm_path(tmp_path):
    from p3achygo_amd import netspec
    from tfm_restatement import fixture_weights
    cfg, W = fixture_weights("test_b2d96h3_tfm")
    path = str(tmp_path / "tfm.p3w")
    netspec.save_p3w(path, cfg, W)
    return path


def test_rule_bit_for_bit_transformer(built, fwd, tmp_path):
    from p3achygo_amd import features
    _check_rule(_tfm_path(tmp_path), features.random_positions(37, seed=63), fwd)


def _int8_scales(path):
    import int8_restatement as ir
    from p3achygo_amd import engine
    cal = engine.HipEngine(path, 64, flags=engine.FLAG_INT8)
    for batch in ir.calibration_batches():
        cal.load_all(batch)
        cal.int8_calibrate()
        for i in range(len(batch)):
            cal.GetBatch(i)
    scales = cal.int8_scales()
    cal.close()
    return scales


def test_rule_bit_for_bit_int8(built, weight_files, fwd):
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c192classic")
    _check_rule(path, features.random_positions(37, seed=64), fwd, flags=engine.FLAG_INT8, scales=_int8_scales(path))


def test_uniform_mask_equals_symmetry_avg(built, weight_files):
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c256btl1")
    pos = features.random_positions(19, seed=65)
    avg = engine.HipEngine(path, 19, flags=engine.FLAG_SYMMETRY_AVG)
    eng = engine.HipEngine(path, 19, flags=engine.FLAG_SYMMETRY_SLOT)
    try:
        avg.set_symmetries(0x81)
        avg.load_all(pos)
        avg.RunInference()
        want, _ = _rows(avg, range(19))
        got, _ = _evaluate(eng, pos, [0x81] * 19)
        assert got.tobytes() == want.tobytes()
        with pytest.raises(engine.EngineError, match="SYMMETRY_AVG"):
            eng.set_symmetries(0x81)
        with pytest.raises(engine.EngineError, match="P3HIP_FLAG_SYMMETRY_SLOT"):
            avg.set_slot_symmetries(0, 0x81)
        for bad in (0, 256, 0x1FF):
            with pytest.raises(engine.EngineError, match="1 .. 255"):
                eng.set_slot_symmetries(0, bad)
        for bad in (-1, 19):
            with pytest.raises(engine.EngineError, match="bad slot"):
                eng.set_slot_symmetries(bad, 1)
        with pytest.raises(engine.EngineError):
            eng.debug_x(8, 256)
    finally:
        avg.close()
        eng.close()


def _played_games(H, rng):
    games = []
    for target in (0, 3, 40, 120):
        g = H.p3host_game_new(7.5)
        color, played = 1, 0
        for _ in range(target * 4):
            if played >= target:
                break
            i, j = (int(v) for v in rng.integers(0, 19, 2))
            if rng.random() < 0.03:
                i, j = 19, 0
            if H.p3host_game_play(g, i, j, color):
                color, played = -color, played + 1
        games.append((g, color))
    return games


def test_single_symmetry_equals_the_host_path(built, weight_files):
    """for each symmetry s: the slot engine fed identity features with mask 1 << s returns the result record of the host
    path, FillFeatures under s -> plain engine -> UnapplySymmetry"""
    from p3achygo_amd import engine, features, host_api
    H = host_api.lib()
    games = _played_games(H, np.random.default_rng(7))
    n = len(games)
    try:
        ident = np.zeros(n, features.features_dtype())
        rot = np.zeros((8, n), features.features_dtype())
        for k, (g, color) in enumerate(games):
            H.p3host_game_features(g, color, 0, ident[k:k + 1].ctypes.data)
            for s in range(8):
                H.p3host_game_features(g, color, s, rot[s, k:k + 1].ctypes.data)
    finally:
        for g, _ in games:
            H.p3host_game_free(g)
    path = weight_files("test_b3c256btl1")
    plain = engine.HipEngine(path, 8 * n)
    eng = engine.HipEngine(path, 8 * n, flags=engine.FLAG_SYMMETRY_SLOT, symmetry_rows=8 * n)
    try:
        for s in range(8):
            for k in range(n):
                plain.LoadBatch(s * n + k, rot[s, k:k + 1])
                eng.LoadBatch(s * n + k, ident[k:k + 1])
                eng.set_slot_symmetries(s * n + k, 1 << s)
        plain.RunInference()
        eng.RunInference()
        for s in range(8):
            for k in range(n):
                want = plain.GetBatch(s * n + k)
                H.p3host_unapply_symmetry(s, C.addressof(want))
                got = eng.GetBatch(s * n + k)
                assert bytes(got) == bytes(want), (s, k)
    finally:
        eng.close()
        plain.close()


def test_compaction_and_run_all_slots(built, weight_files, fwd):
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c256btl1")
    pos = features.random_positions(64, seed=66)
    slots = [0, 3, 4, 9, 17, 18, 22, 29, 31, 32, 40, 41, 47, 50, 55, 62, 63]
    assert len(slots) == 17
    masks = _cycle(17)
    plain = engine.HipEngine(path, 8 * 17)
    want = _restated(plain, pos[slots], masks, fwd)
    ones = _restated(plain, pos[slots], [0x01] * 17, fwd)
    plain.close()
    L = engine.lib()
    for flags in (0, engine.FLAG_RUN_ALL_SLOTS):
        eng = engine.HipEngine(path, 64, flags=engine.FLAG_SYMMETRY_SLOT | flags)
        try:
            _load(eng, pos[slots], masks, slots)
            eng.RunInference()
            got, _ = _rows(eng, slots)
            assert got.tobytes() == want.tobytes(), flags
            if not flags:
                res = (C.c_float * 1892)()
                assert L.p3hip_get_slot(eng._h, 1, C.addressof(res)) == 2
            # loaded again without a new mask: evaluated under 0x01
            for s in slots:
                eng.LoadBatch(s, pos[s:s + 1])
            eng.RunInference()
            got, _ = _rows(eng, slots)
            assert got.tobytes() == ones.tobytes(), flags
        finally:
            eng.close()


def test_capacity(built, weight_files, fwd):
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c256btl1")
    pos = features.random_positions(8, seed=67)
    plain = engine.HipEngine(path, 16)
    eng = engine.HipEngine(path, 8, flags=engine.FLAG_SYMMETRY_SLOT, symmetry_rows=15)
    L = engine.lib()
    try:
        masks = [0xFF, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80]
        got, _ = _evaluate(eng, pos, masks)                        # 8 + 7 = 15 copies: runs
        assert got.tobytes() == _restated(plain, pos, masks, fwd).tobytes()
        masks[1] = 0xFF                                            # 8 + 8 + 6 = 22 copies
        _load(eng, pos, masks)
        assert L.p3hip_run(eng._h) == 1
        msg = L.p3hip_last_error(eng._h).decode()
        assert "22" in msg and "15" in msg, msg
        res = (C.c_float * 1892)()
        for s in range(8):
            assert L.p3hip_get_slot(eng._h, s, C.addressof(res)) == 2
        masks[1] = 0x04
        eng.set_slot_symmetries(1, 0x04)                           # the slots are still pending
        eng.RunInference()
        got, _ = _rows(eng, range(8))
        assert got.tobytes() == _restated(plain, pos, masks, fwd).tobytes()
    finally:
        eng.close()
        plain.close()


def test_nn_cache(built, weight_files, fwd):
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c256btl1")
    pos = features.random_positions(12, seed=68)
    masks = _cycle(12)
    plain = engine.HipEngine(path, 8 * 12)
    want = _restated(plain, pos, masks, fwd)
    plain.close()
    eng = engine.HipEngine(path, 12, flags=engine.FLAG_SYMMETRY_SLOT)
    eng.EnableCache(10)
    try:
        syms = [(3 * i) % 8 for i in range(12)]

        def run(load_syms, these_masks, slots=range(12)):
            for i in slots:
                eng.LoadBatchKeyed(i, pos[i:i + 1], 2000 + i, 9, load_syms[i])
                eng.set_slot_symmetries(i, these_masks[i])
            eng.RunInference()
            out = {}
            for i in slots:
                raw = eng.get_raw(i)
                r, sym, hit = eng.GetBatchKeyed(i)
                out[i] = (sr.row_of(r, raw), sym, hit)
            return out

        first = run(syms, masks)
        for i in range(12):
            row, sym, hit = first[i]
            assert sym == syms[i] and not hit
            assert row.tobytes() == want[i].tobytes(), i
        st = eng.cache_stats()
        assert (st["lookups"], st["hits"], st["stored"]) == (12, 0, 12)
        # the same keys under other loaded symmetries and other masks: served from the table
        again = run([(s + 1) % 8 for s in syms], [0x01] * 12)
        for i in range(12):
            row, sym, hit = again[i]
            assert hit and sym == syms[i]
            assert row.tobytes() == want[i].tobytes(), i
        st = eng.cache_stats()
        assert (st["lookups"], st["hits"], st["stored"]) == (24, 12, 12)
    finally:
        eng.close()


def test_nn_cache_misses_among_hits(built, weight_files, fwd):
    """a run whose misses are a scattered subset: their masks travel with them into the misses' own table"""
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c256btl1")
    pos = features.random_positions(12, seed=69)
    masks = _cycle(12)[::-1]
    plain = engine.HipEngine(path, 8 * 12)
    want = _restated(plain, pos, masks, fwd)
    plain.close()
    eng = engine.HipEngine(path, 12, flags=engine.FLAG_SYMMETRY_SLOT)
    eng.EnableCache(10)
    try:
        def run(slots):
            for i in slots:
                eng.LoadBatchKeyed(i, pos[i:i + 1], 3000 + i, 5, 0)
                eng.set_slot_symmetries(i, masks[i])
            eng.RunInference()
            out = {}
            for i in slots:
                raw = eng.get_raw(i)
                r, _, hit = eng.GetBatchKeyed(i)
                out[i] = (sr.row_of(r, raw), hit)
            return out

        run([0, 2, 5, 7, 8])
        out = run(range(12))
        for i in range(12):
            assert out[i][1] == (i in (0, 2, 5, 7, 8)), i
            assert out[i][0].tobytes() == want[i].tobytes(), i
        # the staged table is the run's again, not the misses': the resident hooks take all 12 slots under their masks
        eng.forward_resident(12)
        eng.sync()
    finally:
        eng.close()


def test_launch_graph(built, weight_files, fwd):
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c256btl1")
    plain = engine.HipEngine(path, 16)
    eng = engine.HipEngine(path, 8, flags=engine.FLAG_SYMMETRY_SLOT | engine.FLAG_LAUNCH_GRAPH)
    try:
        def check(seed, masks):
            pos = features.random_positions(8, seed=seed)
            got, _ = _evaluate(eng, pos, masks)
            assert got.tobytes() == _restated(plain, pos, masks, fwd).tobytes(), (seed, masks)

        check(70, [1 << (i % 8) for i in range(8)])
        check(71, [1 << ((3 * i + 1) % 8) for i in range(8)])
        assert eng.graph_state() == 1
        check(72, [1 << ((5 * i + 2) % 8) for i in range(8)])        # a replay with other symmetries and positions
        assert eng.graph_state() == 1
        check(73, [0x01, 0x02, 0xFF, 0x08, 0x10, 0x20, 0x40, 0x80])  # one averaged slot: kernel by kernel
        check(74, [1 << ((7 * i + 3) % 8) for i in range(8)])
        assert eng.graph_state() == 1
    finally:
        eng.close()
        plain.close()


@pytest.mark.parametrize("net", ["test_b3c256btl1", "test_b2d96h3_tfm"])
def test_low_latency(built, weight_files, fwd, tmp_path, net):
    from p3achygo_amd import engine, features
    path = _tfm_path(tmp_path) if net.endswith("tfm") else weight_files(net)
    pos = features.random_positions(4, seed=75)
    masks = [0xFF, 0x20, 0x81, 0x04]
    plain = engine.HipEngine(path, 12, flags=engine.FLAG_LOW_LATENCY_ANY)
    eng = engine.HipEngine(path, 4, flags=engine.FLAG_LOW_LATENCY_ANY | engine.FLAG_SYMMETRY_SLOT)
    try:
        got, _ = _evaluate(eng, pos, masks)
        assert got.tobytes() == _restated(plain, pos, masks, fwd).tobytes()
    finally:
        eng.close()
        plain.close()


def test_int8_calibration_observes_every_copy(built, weight_files, fwd):
    import int8_restatement as ir
    from p3achygo_amd import engine
    path = weight_files("test_b3c192classic")
    batches = ir.calibration_batches()
    n = max(len(b) for b in batches)
    eng = engine.HipEngine(path, n, flags=engine.FLAG_INT8 | engine.FLAG_SYMMETRY_SLOT)
    plain = engine.HipEngine(path, 8 * n, flags=engine.FLAG_INT8)
    try:
        for b in batches:
            masks = _cycle(len(b))
            _load(eng, b, masks)
            eng.int8_calibrate()
            cp = _copies(b, masks, fwd)
            for i in range(len(cp)):
                plain.LoadBatch(i, cp[i:i + 1])
            plain.int8_calibrate()
            for i in range(len(b)):
                eng.GetBatch(i)
            for i in range(len(cp)):
                plain.GetBatch(i)
        assert np.array_equal(eng.int8_scales(), plain.int8_scales())
        with pytest.raises(engine.EngineError):
            eng.debug_act_i8(4, 192)
    finally:
        eng.close()
        plain.close()


def test_score(built, weight_files, fwd):
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c256btl1")
    n = 9
    pos = features.random_positions(n, seed=76)
    masks = _cycle(n)
    rng = np.random.default_rng(77)
    labels = np.zeros(n, engine.labels_dtype())
    pol = rng.random((n, 362)).astype(np.float32)
    labels["policy"] = pol / pol.sum(1, keepdims=True)
    labels["score_margin"] = rng.integers(-40, 40, n).astype(np.float32) + 0.5
    labels["did_win"] = rng.integers(0, 2, n)
    plain = engine.HipEngine(path, 8 * n)
    eng = engine.HipEngine(path, n, flags=engine.FLAG_SYMMETRY_SLOT)
    try:
        want = _restated(plain, pos, masks, fwd)
        _load(eng, pos, masks)
        for i in range(n):
            eng.load_labels(i, labels[i:i + 1])
        eng.RunInference()
        sums, scored = eng.score()
        assert scored == n
        terms = np.stack([eng.get_score(i) for i in range(n)])
        wt, ws = plain.debug_score_rows(want[:, 362:724], want[:, 724:726], want[:, 726:1526], labels)
        assert terms.tobytes() == wt.tobytes()
        assert np.array_equal(sums, ws)
        with pytest.raises(engine.EngineError, match="P3HIP_FLAG_AUX"):
            eng.loss()
    finally:
        eng.close()
        plain.close()


def _selfplay_records(tmp, weights, device_symmetry):
    """a fixed number of batches of self-play (one group, so the schedule is fixed): the counters, the first games'
    digests, and what the recorder wrote: every game's sgf line and every training record (the per-move search results)"""
    from p3achygo_amd import host_api
    os.makedirs(tmp)
    host_api.set_groups(1)
    host_api.set_step_limit(300)
    host_api.set_recorder(str(tmp), gen=1, worker_id="w", flush_interval=1)
    host_api.set_device_symmetry(device_symmetry)
    try:
        st = host_api.selfplay_run(weights, num_games=8, num_threads=1, seconds=0.0, default_n=8, default_k=4,
                                   selected_n=8, selected_k=4, max_moves=10, warmup_batches=0, seed=21)
        digests = host_api.last_first_game_digests().tolist()
    finally:
        host_api.set_device_symmetry(0)
        host_api.set_recorder("")
        host_api.set_step_limit(0)
        host_api.set_groups(2)
    # what was recorded, whatever batch file it landed in (flushes go by the clock): the sgf line of every game and
    # every training record (TFRecord framing: u64 length, u32 crc, payload, u32 crc) of every chunk
    import zlib
    games, records = [], []
    for root, _, names in os.walk(tmp):
        for nm in names:
            with open(os.path.join(root, nm), "rb") as f:
                data = f.read()
            if nm.endswith(".sgf"):
                games += [ln for ln in data.split(b"\n") if ln]
            elif nm.endswith(".tfrecord.zz"):
                raw, at = zlib.decompress(data), 0
                while at < len(raw):
                    n = int.from_bytes(raw[at:at + 8], "little")
                    records.append(raw[at + 12:at + 12 + n])
                    at += 16 + n
                assert at == len(raw)
    return (st.positions, st.moves, st.games, st.black_wins, st.cache_hits), digests, sorted(games), sorted(records)


def test_selfplay_with_device_symmetry_plays_the_host_paths_games(built, weight_files, tmp_path):
    w = weight_files("test_b3c128btl2")
    host = _selfplay_records(tmp_path / "host", w, 0)
    dev = _selfplay_records(tmp_path / "dev", w, 1)
    assert host[0][2] >= 8 and all(host[1]) and len(host[1]) == 8      # every runner finished a game
    assert len(host[2]) >= 8 and len(host[3]) > 0                       # games and per-move training records
    assert dev[0] == host[0]
    assert dev[1] == host[1]
    assert dev[2] == host[2]
    assert dev[3] == host[3]


def _eval_games(tmp, weights, cur="", cand="", **kw):
    """the sgf lines (one per game) and the counters of one scheduler-driven eval match"""
    from p3achygo_amd import host_api
    try:
        host_api.eval_set_player_flags(cur=cur, cand=cand)
        host_api.eval_set_paths(recorder_dir=str(tmp))
        st = host_api.eval_match(weights, weights, num_games=4, visits_per_move=12, leaves_per_round=4, max_moves=10,
                                 num_threads=2, seed=9, **kw)
    finally:
        host_api.eval_set_player_flags()
        host_api.eval_set_paths()
    lines = []
    for f in sorted((tmp / "sgf").iterdir()):
        if f.name.endswith(".sgf"):
            lines += f.read_text().splitlines()
    return lines, (st.games, st.moves, st.visits, st.positions, st.cur_wins, st.cand_wins)


def test_eval_match_with_device_symmetry_plays_the_host_paths_games(built, weight_files, tmp_path):
    """both players hand their random symmetries to the engine: the same draws, bit-identical results, so the same match"""
    w = weight_files("test_b3c128btl2")
    host = _eval_games(tmp_path / "host", w)
    dev = _eval_games(tmp_path / "dev", w, cur="nn_device_symmetry: 1\n", cand="nn_device_symmetry: 1\n")
    assert host[1][0] == 4 and len(host[0]) == 4
    assert dev == host


def test_eval_match_with_a_root_mask_plays_the_same_games_twice(built, weight_files, tmp_path):
    w = weight_files("test_b3c128btl2")
    a = _eval_games(tmp_path / "a", w, cand="nn_root_symmetry_mask: 0xFF\n")
    b = _eval_games(tmp_path / "b", w, cand="nn_root_symmetry_mask: 0xFF\n")
    assert a[1][0] == 4 and a[1][1] == 4 * 10 and len(a[0]) == 4
    assert a == b


def test_eval_match_threads_with_a_root_mask(built, weight_files):
    """the thread-per-game driver: ThreadedSearch marks its root visit, NNInterface hands the root mask over; the
    engine has batch + 7 x games rows"""
    from p3achygo_amd import host_api
    w = weight_files("test_b3c128btl2")
    try:
        host_api.eval_set_player_flags(cur="nn_device_symmetry: 1\n", cand="nn_root_symmetry_mask: 0xFF\n")
        st = host_api.eval_match_threads(w, w, num_games=2, visits_per_move=8, threads_per_game=2, max_moves=12, seed=5)
    finally:
        host_api.eval_set_player_flags()
    assert st.games == 2 and st.moves == 2 * 12 and st.visits > 0
