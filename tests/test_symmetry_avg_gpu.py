"""Symmetry-averaged evaluation on the MI355X (P3HIP_FLAG_SYMMETRY_AVG).

The restatement of a flagged engine's result is a plain engine run over the copies that the CPU-pinned numpy expand
makes (tests/symavg_restatement.py), its rows un-rotated and averaged in numpy float32 in the stated order.  Every
output float must equal it bit for bit: the forward pass of a row does not depend on the other rows of its batch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import symavg_restatement as sr  # noqa: E402

pytestmark = pytest.mark.gpu

MASKS = (0x01, 0x10, 0x81, 0xFF)


@pytest.fixture(scope="module")
def fwd(built):
    from p3achygo_amd import engine
    return engine.symmetry_maps()[0]


def _rows(eng, slots):
    """(rows, ownership maps) of `slots` after a run, fetched the way a host fetches them"""
    rows, owns = [], []
    for s in slots:
        raw = eng.get_raw(s)
        owns.append(eng.GetOwnership(s))
        rows.append(sr.row_of(eng.GetBatch(s), raw))
    return np.stack(rows), np.stack(owns)


def _evaluate(eng, recs):
    eng.load_all(recs)
    eng.RunInference()
    return _rows(eng, range(len(recs)))


def _restated(plain, pos, mask, fwd):
    k = len(sr.syms_of(mask))
    rows, _ = _evaluate(plain, sr.expand(pos, mask, fwd))
    return np.stack([sr.reduce(list(rows[i * k:(i + 1) * k]), mask, fwd) for i in range(len(pos))])


def _check_rule(path, pos, fwd, masks=MASKS, flags=0, scales=None):
    from p3achygo_amd import engine
    n = len(pos)
    plain = engine.HipEngine(path, 8 * n, flags=flags)
    eng = engine.HipEngine(path, n, flags=flags | engine.FLAG_SYMMETRY_AVG)
    try:
        if scales is not None:
            plain.set_int8_scales(scales)
            eng.set_int8_scales(scales)
        for mask in masks:
            eng.set_symmetries(mask)
            got, own = _evaluate(eng, pos)
            want = _restated(plain, pos, mask, fwd)
            assert got.tobytes() == want.tobytes(), (hex(mask), np.argwhere(got != want)[:5])
            assert own.tobytes() == got[:, sr.OWNERSHIP].tobytes()
            if mask == 0x01:   # one symmetry: the plain engine itself
                ref, _ = _evaluate(plain, pos)
                assert got.tobytes() == ref.tobytes()
    finally:
        eng.close()
        plain.close()


def test_rule_bit_for_bit(built, weight_files, fwd):
    from p3achygo_amd import features
    _check_rule(weight_files("test_b3c256btl1"), features.random_positions(37, seed=41), fwd)


def test_rule_bit_for_bit_b12c256btl3_1024_slots(built, weight_files, fwd):
    from p3achygo_amd import features
    _check_rule(weight_files("b12c256btl3"), features.random_positions(1024, seed=42), fwd, masks=(0x01, 0x81, 0xFF))


def test_rule_bit_for_bit_c384(built, weight_files, fwd):
    from p3achygo_amd import features
    _check_rule(weight_files("test_b3c384btl3"), features.random_positions(37, seed=43), fwd)


def test_rule_bit_for_bit_int8(built, weight_files, fwd):
    import int8_restatement as ir
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c192classic")
    cal = engine.HipEngine(path, 64, flags=engine.FLAG_INT8)
    for batch in ir.calibration_batches():
        cal.load_all(batch)
        cal.int8_calibrate()
        for i in range(len(batch)):
            cal.GetBatch(i)
    scales = cal.int8_scales()
    cal.close()
    _check_rule(path, features.random_positions(37, seed=44), fwd, flags=engine.FLAG_INT8, scales=scales)


def test_rule_bit_for_bit_transformer(built, fwd, tmp_path):
    from p3achygo_amd import features, netspec
    from tfm_restatement import fixture_weights
    cfg, W = fixture_weights("test_b2d96h3_tfm")
    path = str(tmp_path / "tfm.p3w")
    netspec.save_p3w(path, cfg, W)
    _check_rule(path, features.random_positions(37, seed=45), fwd)


def test_int8_calibration_observes_every_copy(built, weight_files, fwd):
    """p3hip_int8_calibrate on a flagged engine folds the maxima of all k copies: the scales equal those of a plain
    engine calibrated on the copies themselves."""
    import int8_restatement as ir
    from p3achygo_amd import engine
    path = weight_files("test_b3c192classic")
    batches = ir.calibration_batches()
    n = max(len(b) for b in batches)
    eng = engine.HipEngine(path, n, flags=engine.FLAG_INT8 | engine.FLAG_SYMMETRY_AVG)
    plain = engine.HipEngine(path, 8 * n, flags=engine.FLAG_INT8)
    try:
        eng.set_symmetries(0x81)
        for b in batches:
            eng.load_all(b)
            eng.int8_calibrate()
            cp = sr.expand(b, 0x81, fwd)
            plain.load_all(cp)
            plain.int8_calibrate()
            for i in range(len(b)):
                eng.GetBatch(i)
            for i in range(len(cp)):
                plain.GetBatch(i)
        assert np.array_equal(eng.int8_scales(), plain.int8_scales())
    finally:
        eng.close()
        plain.close()


def _logit_mask():
    """row entries that are probabilities or ownership (the rest: logits, err2, gamma)"""
    m = np.zeros(sr.OUT_STRIDE, bool)
    m[362:1526] = True      # move probs, value probs, score probs
    m[1526:1888] = True     # opt probs
    m[sr.OWNERSHIP] = True
    return m


def test_invariance_under_the_symmetries(built, weight_files, fwd):
    """mask 0xFF: the result for P and the un-rotated result for P under each symmetry are averages over the same set
    of copies, in a different order"""
    from p3achygo_amd import engine, features
    pos = features.random_positions(6, seed=46)
    rot = sr.expand(pos, 0xFF, fwd)    # P under every symmetry, rows 8 p + s
    eng = engine.HipEngine(weight_files("test_b3c256btl1"), len(rot), flags=engine.FLAG_SYMMETRY_AVG)
    try:
        rows, _ = _evaluate(eng, rot)
    finally:
        eng.close()
    probs = _logit_mask()
    for p in range(len(pos)):
        base = rows[8 * p]
        assert np.abs(base[probs]).max() > 0
        for s in range(1, 8):
            un = sr.unrotate(rows[8 * p + s], s, fwd)
            d = np.abs(un - base)
            assert d[probs].max() <= 1e-6, (p, s, d[probs].max())
            assert (d[~probs] <= 1e-5 * np.maximum(1.0, np.abs(base[~probs]))).all(), (p, s)


def test_compaction_and_run_all_slots(built, weight_files, fwd):
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c256btl1")
    pos = features.random_positions(16, seed=47)
    full = engine.HipEngine(path, 16, flags=engine.FLAG_SYMMETRY_AVG)
    want, _ = _evaluate(full, pos)
    full.close()
    L = engine.lib()
    for flags in (0, engine.FLAG_RUN_ALL_SLOTS):
        eng = engine.HipEngine(path, 16, flags=engine.FLAG_SYMMETRY_AVG | flags)
        try:
            for ragged in ([3], [0, 5, 6, 11, 15], list(range(1, 16, 2))):
                for s in ragged:
                    eng.LoadBatch(s, pos[s:s + 1])
                eng.RunInference()
                got, _ = _rows(eng, ragged)
                assert got.tobytes() == want[ragged].tobytes(), (flags, ragged)
                if not flags:
                    res = (C.c_float * 1892)()
                    other = next(s for s in range(16) if s not in ragged)
                    assert L.p3hip_get_slot(eng._h, other, C.addressof(res)) == 2
        finally:
            eng.close()


def test_nn_cache_serves_the_averaged_results(built, weight_files, fwd):
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c256btl1")
    pos = features.random_positions(12, seed=48)
    plain_avg = engine.HipEngine(path, 12, flags=engine.FLAG_SYMMETRY_AVG)
    want, _ = _evaluate(plain_avg, pos)
    plain_avg.close()
    eng = engine.HipEngine(path, 12, flags=engine.FLAG_SYMMETRY_AVG)
    eng.EnableCache(10)
    try:
        syms = [(3 * i) % 8 for i in range(12)]
        for i in range(12):
            eng.LoadBatchKeyed(i, pos[i:i + 1], 1000 + i, 7, syms[i])
        eng.RunInference()
        first = []
        for i in range(12):
            raw = eng.get_raw(i)
            r, sym, hit = eng.GetBatchKeyed(i)
            assert sym == syms[i] and not hit
            first.append(sr.row_of(r, raw))
        first = np.stack(first)
        assert first.tobytes() == want.tobytes()                 # the misses: the averaged results
        for i in range(12):                                       # the same keys, loaded under other symmetries
            eng.LoadBatchKeyed(i, pos[i:i + 1], 1000 + i, 7, (syms[i] + 1) % 8)
        eng.RunInference()
        for i in range(12):
            raw = eng.get_raw(i)
            r, sym, hit = eng.GetBatchKeyed(i)
            assert hit and sym == syms[i]                          # the stored result and the symmetry it was loaded in
            assert sr.row_of(r, raw).tobytes() == first[i].tobytes()
        assert eng.cache_stats()["hits"] == 12
    finally:
        eng.close()


def test_launch_graph(built, weight_files, fwd):
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c256btl1")
    pos = features.random_positions(16, seed=49)
    plain = engine.HipEngine(path, 8 * 16)
    eng = engine.HipEngine(path, 16, flags=engine.FLAG_SYMMETRY_AVG | engine.FLAG_LAUNCH_GRAPH)
    try:
        want = _restated(plain, pos, 0xFF, fwd)
        for _ in range(4):
            got, _ = _evaluate(eng, pos)
            assert got.tobytes() == want.tobytes()
        assert eng.graph_state() == 1
        eng.set_symmetries(0x0F)
        want = _restated(plain, pos, 0x0F, fwd)
        for _ in range(3):
            got, _ = _evaluate(eng, pos)
            assert got.tobytes() == want.tobytes()
        assert eng.graph_state() == 1
    finally:
        eng.close()
        plain.close()


def test_errors_and_measurement_hooks(built, weight_files, fwd):
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c256btl1")
    eng = engine.HipEngine(path, 8, flags=engine.FLAG_SYMMETRY_AVG)
    plain = engine.HipEngine(path, 8)
    try:
        for bad in (0, 256, 0x1FF):
            with pytest.raises(engine.EngineError, match="1 .. 255"):
                eng.set_symmetries(bad)
        with pytest.raises(engine.EngineError, match="SYMMETRY_AVG"):
            plain.set_symmetries(0xFF)
        with pytest.raises(engine.EngineError, match="row limit"):
            engine.HipEngine(path, 8193, flags=engine.FLAG_SYMMETRY_AVG)
        engine.HipEngine(path, 8192, flags=engine.FLAG_SYMMETRY_AVG).close()
        # the measurement hooks count slots: upload + forward_resident leave the averaged rows in d_out
        pos = features.random_positions(8, seed=50)
        want, _ = _evaluate(eng, pos)
        eng.load_all(pos)
        eng.upload()
        eng.forward_resident(8)
        eng.sync()
        got = np.stack([eng.get_raw(i) for i in range(8)])
        assert np.array_equal(got[:, 362:724], want[:, 1889:2251])
        ms, fl, name = eng.time_trunk_kernel(8, 2)
        assert ms > 0 and name
        with pytest.raises(engine.EngineError):
            eng.debug_x(8, 256)
    finally:
        eng.close()
        plain.close()


def test_eval_match_threads_with_symmetry_averaging(built, weight_files):
    from p3achygo_amd import host_api
    w = weight_files("test_b3c128btl2")
    try:
        host_api.eval_set_player_flags(cand="nn_symmetry_mask: 255\n")
        st = host_api.eval_match_threads(w, w, num_games=2, visits_per_move=8, threads_per_game=2, max_moves=12,
                                         seed=5)
    finally:
        host_api.eval_set_player_flags()
    assert st.games == 2 and st.moves == 2 * 12 and st.visits > 0
