"""Scoring against labels on the MI355X (csrc/score.hip behind p3hip_load_labels / p3hip_score / p3hip_get_score /
p3hip_debug_score_rows) and calibration from recorded chunks (p3achygo_amd/dataset.py).

The reference is tests/dataset_restatement.py: hits, score_pred and score_diff must be equal, the two losses within
2 fp32 ulp of the float64 -log(p) (the HIP math library documents 1 ulp for logf; the comparison rounds once more),
every sum within n * 2^-52 * sum |term| of numpy's float64 sum of the returned terms and bit-identical on a repeat.

Measured on one MI355X: the largest loss distance is 0.498 ulp over the synthetic rows and 0.496 ulp over the end-to-end,
composition and calibration cases (the kernel takes the logarithm in double and rounds once; with the device's logf
these rows gave 1.94 ulp and a sweep of other probabilities 2.08).  Every sum met its bound and
repeated bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dataset_common as dc  # noqa: E402
import dataset_restatement as dr  # noqa: E402

pytestmark = pytest.mark.gpu

NET, BATCH = "test_b3c128btl2", 96
GAMES = 3


@pytest.fixture(scope="module")
def chunk(built, tmp_path_factory):
    """(path, features, labels) of a chunk the recorder wrote: GAMES copies of the scripted game."""
    from p3achygo_amd import dataset
    path = dc.record_game(tmp_path_factory.mktemp("chunk"), games=GAMES)
    ds = dataset.Dataset(path)
    assert len(ds) == GAMES * len(dc.GAME)
    return path, ds.features, ds.labels


# ---- synthetic rows ------------------------------------------------------------------------------
_synthetic = dc.synthetic_rows


@pytest.fixture(scope="module")
def small_engine(built, weight_files):
    from p3achygo_amd import engine
    eng = engine.HipEngine(weight_files(NET), BATCH)
    yield eng
    eng.close()


def _check_sums(sums, terms, n):
    t64 = np.asarray(terms, np.float64)
    for j in range(6):
        want = t64[:, j].sum()
        bound = n * 2.0 ** -52 * np.abs(t64[:, j]).sum()
        assert abs(sums[j] - want) <= bound, (dr.TERMS[j], sums[j], want, bound)


@pytest.mark.parametrize("n", [1, 5, 64, 65, 96])
def test_synthetic_rows(small_engine, n):
    mp, vp, sp, lab = (a[:n] for a in _synthetic())
    terms, sums = small_engine.debug_score_rows(mp, vp, sp, lab)
    want = dr.terms_rows(mp, vp, sp, lab)
    worst = dr.check_against(terms, want)
    print(f"n {n}: largest loss distance {worst:.3f} ulp; sums {sums}")
    assert np.isfinite(terms).all()
    _check_sums(sums, terms, n)
    terms2, sums2 = small_engine.debug_score_rows(mp, vp, sp, lab)
    assert terms2.tobytes() == terms.tobytes() and sums2.tobytes() == sums.tobytes()
    if n >= 18:     # every pattern is there: the branches the rows were built for were taken
        assert set(want[:, 5]) >= {-399.0, -1.0, 0.0, 1.0, 399.0} and (want[:, :2] == 16.0).any(axis=0).all()
        assert {0.0, 1.0} == set(want[:, 2]) == set(want[:, 3])


def test_debug_score_rows_refuses_bad_counts(small_engine):
    from p3achygo_amd import engine
    mp, vp, sp, lab = _synthetic(BATCH + 1)
    with pytest.raises(engine.EngineError):
        small_engine.debug_score_rows(mp, vp, sp, lab)
    with pytest.raises(engine.EngineError):
        small_engine.debug_score_rows(mp[:0], vp[:0], sp[:0], lab[:0])


# ---- end to end ----------------------------------------------------------------------------------
def _check_slots(eng, slots, labels):
    """get_score of every slot against the restatement on the slot's own GetBatch result; returns the terms."""
    got, want = [], []
    for k, s in enumerate(slots):
        t = eng.get_score(s)
        assert t is not None, s
        r = eng.GetBatch(s)
        want.append(dr.terms(np.ctypeslib.as_array(r.move_probs), np.ctypeslib.as_array(r.value_probs),
                             np.ctypeslib.as_array(r.score_probs), labels["policy"][k], labels["score_margin"][k],
                             labels["did_win"][k]))
        got.append(t)
    worst = dr.check_against(np.stack(got), np.stack(want))
    print(f"largest loss distance {worst:.3f} ulp")
    return np.stack(got)


@pytest.mark.parametrize("run_all", [False, True])
def test_end_to_end_on_a_recorded_chunk(built, weight_files, chunk, run_all):
    from p3achygo_amd import engine
    _, feats, labels = chunk
    n = len(feats)
    slots = [3 * k for k in range(n)]          # scattered: row != slot once the run compacts
    assert slots[-1] < BATCH
    eng = engine.HipEngine(weight_files(NET), BATCH, flags=engine.FLAG_RUN_ALL_SLOTS if run_all else 0)
    try:
        assert eng.score()[1] == 0             # nothing loaded yet
        for k, s in enumerate(slots):
            eng.LoadBatch(s, feats[k:k + 1])
            eng.load_labels(s, labels[k:k + 1])
        eng.LoadBatch(1, feats[0:1])           # evaluated, but without labels
        eng.load_labels(4, labels[0:1])
        eng.LoadBatch(4, feats[1:2])           # a new load clears the labels given before it
        eng.RunInference()
        sums, scored = eng.score()
        assert scored == n
        assert eng.get_score(1) is None and eng.get_score(4) is None
        assert eng.get_score(2) is None        # not loaded (RUN_ALL_SLOTS evaluates it all the same: still no labels)
        if not run_all:
            with pytest.raises(engine.EngineError):
                eng.GetBatch(2)
        terms = _check_slots(eng, slots, labels)
        _check_sums(sums, terms, n)
        sums2, scored2 = eng.score()           # after every slot was fetched: the same rows, the same bits
        assert scored2 == n and sums2.tobytes() == sums.tobytes()
        assert np.stack([eng.get_score(s) for s in slots]).tobytes() == terms.tobytes()
        # the next run ends it: slot 0 reloaded without labels, the others not part of the run
        eng.GetBatch(1), eng.GetBatch(4)
        if run_all:
            eng.GetBatch(2)
        eng.LoadBatch(0, feats[0:1])
        eng.RunInference()
        assert eng.get_score(3) is None
        sums3, scored3 = eng.score()
        assert scored3 == (n - 1 if run_all else 0) and eng.get_score(0) is None
        assert (eng.get_score(3) is not None) == run_all
    finally:
        eng.close()


def test_a_slot_loaded_again_after_the_run_is_left_out_and_hooks_end_the_scoring(built, weight_files, chunk):
    """Labels pair with the row of the load the run evaluated: a slot reloaded (with labels) between run and score is not
    scored.  p3hip_forward_resident and p3hip_debug_score_rows overwrite the output rows: nothing is scored after them
    until the next run."""
    from p3achygo_amd import engine
    _, feats, labels = chunk
    eng = engine.HipEngine(weight_files(NET), BATCH)
    try:
        for s in range(4):
            eng.LoadBatch(s, feats[s:s + 1])
            eng.load_labels(s, labels[s:s + 1])
        eng.RunInference()
        eng.LoadBatch(2, feats[9:10])
        eng.load_labels(2, labels[9:10])
        sums, scored = eng.score()
        assert scored == 3 and eng.get_score(2) is None and eng.get_score(3) is not None
        _check_slots(eng, [0, 1, 3], labels[[0, 1, 3]])
        eng.RunInference()                       # slot 2's new load: evaluated and scored now
        assert eng.get_score(3) is None
        sums, scored = eng.score()
        assert scored == 1
        t2 = eng.get_score(2)
        eng.forward_resident(4)
        eng.sync()
        assert eng.get_score(2) is None and eng.score()[1] == 0
        eng.LoadBatch(2, feats[9:10])
        eng.load_labels(2, labels[9:10])
        eng.RunInference()
        assert eng.score()[1] == 1 and eng.get_score(2).tobytes() == t2.tobytes()
        mp, vp, sp, lab = (a[:2] for a in dc.synthetic_rows())
        eng.debug_score_rows(mp, vp, sp, lab)
        assert eng.get_score(2) is None and eng.score()[1] == 0
    finally:
        eng.close()


# ---- the tool ------------------------------------------------------------------------------------
def test_dataset_benchmark_tool_runs_every_plan_and_the_ab(built, weight_files, chunk, tmp_path, capsys):
    """tools/dataset_benchmark.py end to end on the small net: fp16, fp32 and the INT8 plan that serves the trunk
    (calibrated from the chunk), device and host scoring, and the interleaved A/B; the two ways of scoring agree."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("dataset_benchmark", os.path.join(dc.ROOT, "tools", "dataset_benchmark.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path, feats, _ = chunk
    out, ab = str(tmp_path / "bench.jsonl"), str(tmp_path / "ab.jsonl")
    common = [weight_files(NET), path, "--batch", "16", "--warmup", "2", "--out", out, "--ab-out", ab]
    tool.main(common + ["--plans", "fp16,fp32,int8", "--calibrate", path, "--ab", "1"])
    tool.main(common + ["--plans", "fp16", "--host-scoring"])
    text = capsys.readouterr().out
    for line in ("Avg Inference Time:", "Avg Policy Loss:", "Avg Outcome Loss:", "Correct Move Percentage:",
                 "Correct Outcome Percentage:", "Mean Score Diff:"):
        assert text.count(line) == 4, line
    recs = [json.loads(l) for l in open(out)]
    assert [(r["plan"], r["scoring"]) for r in recs] == [("fp16", "device"), ("fp32", "device"), ("int8", "device"), ("fp16", "host")]
    assert recs[2]["flags"] == tool.engine.FLAG_INT8_C128 and recs[2]["calibration_batches"] == 2
    for r in recs:
        assert r["positions"] == len(feats) and r["batches"] == 2 and r["stats"]["num_examples"] == len(feats)
        assert 0 <= r["stats"]["policy_percent"] <= 1 and r["stats"]["policy_loss"] > 0
    for k in ("policy_percent", "outcome_percent", "score_diff", "score_pred_mean"):
        assert recs[0]["stats"][k] == recs[3]["stats"][k], k            # exact terms: device and host agree
    assert recs[0]["stats"]["policy_loss"] == pytest.approx(recs[3]["stats"]["policy_loss"], rel=1e-6)
    abs_ = [json.loads(l) for l in open(ab)]
    assert [r["plan"] for r in abs_] == ["fp16", "fp32", "int8"] and all(r["sums_agree"] for r in abs_)
    assert all(r["device_positions_per_s"] > 0 and r["host_positions_per_s"] > 0 for r in abs_)


# ---- composition ---------------------------------------------------------------------------------
def test_nn_cache_hits_are_scored_like_evaluated_rows(built, weight_files, chunk):
    from p3achygo_amd import engine
    _, feats, labels = chunk
    n = len(dc.GAME)                           # one game's rows: distinct positions, distinct keys
    slots = [3 * k + 1 for k in range(n)]
    eng = engine.HipEngine(weight_files(NET), BATCH)
    try:
        eng.EnableCache(10)

        def run():
            for k, s in enumerate(slots):
                eng.LoadBatchKeyed(s, feats[k:k + 1], 1000 + k, 77, symmetry=0)
                eng.load_labels(s, labels[k:k + 1])
            eng.RunInference()
            sums, scored = eng.score()
            assert scored == n
            return sums, _check_slots(eng, slots, labels)

        sums1, terms1 = run()
        assert eng.cache_stats()["hits"] == 0
        sums2, terms2 = run()
        assert eng.cache_stats()["hits"] == n   # the second run is all hits
        assert sums2.tobytes() == sums1.tobytes() and terms2.tobytes() == terms1.tobytes()
    finally:
        eng.close()


@pytest.mark.parametrize("flag", ["FLAG_SYMMETRY_AVG", "FLAG_FP32"])
def test_scores_follow_the_engines_own_results(built, weight_files, chunk, flag):
    """Symmetry averaging (mask 0x03): the averaged rows are scored.  fp32 plan: that engine's rows."""
    from p3achygo_amd import engine
    _, feats, labels = chunk
    n = len(feats)
    slots = [95 - 3 * k for k in range(n)]
    eng = engine.HipEngine(weight_files(NET), BATCH, flags=getattr(engine, flag))
    try:
        if flag == "FLAG_SYMMETRY_AVG":
            eng.set_symmetries(0x03)
        for k, s in enumerate(slots):
            eng.LoadBatch(s, feats[k:k + 1])
            eng.load_labels(s, labels[k:k + 1])
        eng.RunInference()
        sums, scored = eng.score()
        assert scored == n
        _check_sums(sums, _check_slots(eng, slots, labels), n)
    finally:
        eng.close()


# ---- calibration from chunks ---------------------------------------------------------------------
def test_calibrate_from_chunks_equals_the_hand_written_loop(built, weight_files, chunk):
    from p3achygo_amd import dataset, engine
    path, feats, labels = chunk
    B = 16
    eng = engine.HipEngine(weight_files(NET), B, flags=engine.FLAG_INT8_C128)
    ref = engine.HipEngine(weight_files(NET), B, flags=engine.FLAG_INT8_C128)
    try:
        assert dataset.calibrate_from_chunks(eng, [path]) == -(-len(feats) // B)
        for lo in range(0, len(feats), B):
            part = feats[lo:lo + B]
            for i in range(len(part)):
                ref.LoadBatch(i, part[i:i + 1])
            ref.int8_calibrate()
            for i in range(len(part)):
                ref.GetBatch(i)
        scales = eng.int8_scales()
        assert len(scales) > 0 and (scales > 0).all() and scales.tobytes() == ref.int8_scales().tobytes()
        m = min(B, len(feats))
        dataset.load_batch(eng, feats[:m], labels[:m])
        eng.RunInference()
        sums, scored = eng.score()
        assert scored == m
        _check_sums(sums, _check_slots(eng, range(m), labels[:m]), m)
        stats = dataset.score_chunks(eng, [path], max_batches=2)
        assert stats["num_examples"] == min(2 * B, len(feats)) and 0 <= stats["policy_percent"] <= 1
    finally:
        eng.close()
        ref.close()
