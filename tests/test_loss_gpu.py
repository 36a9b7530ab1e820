"""The trainer's validation losses on the MI355X (csrc/loss.hip behind p3hip_load_targets / p3hip_loss / p3hip_get_loss /
p3hip_debug_loss_rows, dataset.loss_chunks).

The reference is tests/loss_restatement.py in float64 on the same arrays.  Terms 0-16 must lie within
max(4 x the float32 twin's largest distance from float64 on these inputs, 1e-6 max(1, |value|)): the twin is the same
formulas in numpy float32, the factor 4 allows another summation order over up to 800 addends, the floor is 16 float32
roundings.  Terms 17-18 are exact.  Sums equal the float64 sum of the returned terms to 1e-12 relative and repeat bit for
bit.

Measured on one MI355X (the kernel's arithmetic is double, every term rounded to float once): over the synthetic rows no
term is further from float64 than the twin is (ratios 0.085 to 1, allowed 4), and the largest error is 0.046 of its bound;
end to end on the four plans the ratios are 0.004 to 1 and the largest error 0.05 of its bound.  Every sum met its bound and repeated bit for bit.  DESIGN.md
section 14 has the table."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dataset_common as dc  # noqa: E402
import loss_restatement as lr  # noqa: E402

pytestmark = pytest.mark.gpu

NET, BATCH = "test_b3c128btl2", 8


@pytest.fixture(scope="module")
def rows(built, tmp_path_factory):
    """(features, labels, targets) of eight positions: the six fixture rows and two rows of a recorded chunk."""
    from p3achygo_amd import dataset
    fx = dataset.Dataset(dc.FIXTURE)
    rec = dataset.Dataset(dc.record_game(tmp_path_factory.mktemp("chunk")))
    assert fx.has_targets.all() and rec.has_targets.all()
    pick = [4, 7]                      # a white and a black move of the scripted game, stones on the board
    return (np.concatenate([fx.features, rec.features[pick]]), np.concatenate([fx.labels, rec.labels[pick]]),
            np.concatenate([fx.targets, rec.targets[pick]]))


@pytest.fixture(scope="module")
def aux_engine(built, weight_files):
    from p3achygo_amd import engine
    eng = engine.HipEngine(weight_files(NET), BATCH, flags=engine.FLAG_AUX)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def net_file(built, tmp_path_factory):
    """name -> path of a seeded random-init .p3w of any config netspec knows (the transformer tables included)."""
    from p3achygo_amd import netspec
    d, cache = tmp_path_factory.mktemp("loss_weights"), {}

    def get(name):
        if name not in cache:
            cfg = netspec.get_config(name)
            cache[name] = os.path.join(d, name + ".p3w")
            netspec.save_p3w(cache[name], cfg, netspec.generate_weights(cfg, randomize=True))
        return cache[name]
    return get


def _check_sums(sums, terms):
    t64 = np.asarray(terms, np.float64)
    want = t64.sum(axis=0)
    assert (np.abs(sums - want) <= 1e-12 * np.abs(t64).sum(axis=0)).all(), (sums, want)


def _check_slots(eng, slots, targets, label):
    """get_loss of every slot against the restatement on the slot's own get_raw + GetAux; returns the terms."""
    raw = np.stack([eng.get_raw(s) for s in slots])
    aux = np.stack([eng.GetAux(s) for s in slots])
    got = []
    for s in slots:
        t = eng.get_loss(s)
        assert t is not None, s
        got.append(t)
    want, bound, dev = lr.bounds(raw, aux, targets)
    lr.check_against(np.stack(got), want, bound, dev, label)
    assert (np.stack(got)[:, 17:] == want[:, 17:]).all()
    return np.stack(got)


# ---- 1. synthetic rows at trained-net magnitudes ---------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8])
def test_synthetic_rows(aux_engine, n):
    from p3achygo_amd import engine
    raw, aux, tg = (a[:n] for a in lr.synthetic(engine.targets_dtype(), 8))
    terms, sums = aux_engine.debug_loss_rows(raw, aux, tg)
    want, bound, dev = lr.bounds(raw, aux, tg)
    lr.check_against(terms, want, bound, dev, f"n={n}")
    assert (terms[:, 17:] == want[:, 17:]).all()          # the hits are exact, the tie of row 4 on the lower index
    _check_sums(sums, terms)
    terms2, sums2 = aux_engine.debug_loss_rows(raw, aux, tg)
    assert terms2.tobytes() == terms.tobytes() and sums2.tobytes() == sums.tobytes()


def test_debug_loss_rows_refuses_bad_arguments(aux_engine):
    from p3achygo_amd import engine
    raw, aux, tg = lr.synthetic(engine.targets_dtype(), BATCH + 1)
    with pytest.raises(engine.EngineError):
        aux_engine.debug_loss_rows(raw, aux, tg)
    with pytest.raises(engine.EngineError):
        aux_engine.debug_loss_rows(raw[:0], aux[:0], tg[:0])
    tg["policy_aux"][1] = 362
    with pytest.raises(engine.EngineError, match="policy_aux"):
        aux_engine.debug_loss_rows(raw[:2], aux[:2], tg[:2])
    with pytest.raises(engine.EngineError, match="policy_aux"):
        aux_engine.load_targets(0, tg[1:2])


# ---- 2. and 4. end to end, on every kind of plan ---------------------------------------------------
def _end_to_end(net_file, rows, net, flags, calibrate):
    from p3achygo_amd import engine
    feats, labels, targets = rows
    eng = engine.HipEngine(net_file(net), BATCH, flags=flags)
    plain = engine.HipEngine(net_file(net), BATCH, flags=flags)
    try:
        assert eng.loss()[1] == 0                          # nothing loaded yet
        for s in range(BATCH):
            for e in (eng, plain):
                e.LoadBatch(s, feats[s:s + 1])
                e.load_labels(s, labels[s:s + 1])
            eng.load_targets(s, targets[s:s + 1])
        for e in (eng, plain):
            if calibrate:
                e.int8_calibrate()
            e.RunInference()
        sums, n = eng.loss()
        assert n == BATCH
        terms = _check_slots(eng, range(BATCH), targets, f"{net} flags={flags}")
        _check_sums(sums, terms)
        sums2, n2 = eng.loss()
        assert n2 == n and sums2.tobytes() == sums.tobytes()
        # targets change nothing else: the scores and every fetched result keep the bits of an engine without them
        sc, sp = eng.score(), plain.score()
        assert sc[1] == sp[1] == BATCH and sc[0].tobytes() == sp[0].tobytes()
        for s in range(BATCH):
            assert eng.get_raw(s).tobytes() == plain.get_raw(s).tobytes() and eng.GetAux(s).tobytes() == plain.GetAux(s).tobytes()
            assert eng.get_score(s).tobytes() == plain.get_score(s).tobytes()
            assert eng.GetOwnership(s).tobytes() == plain.GetOwnership(s).tobytes()
            assert bytes(eng.GetBatch(s)) == bytes(plain.GetBatch(s))
        assert plain.loss()[1] == 0 and plain.get_loss(0) is None
        sums3, n3 = eng.loss()                             # after every slot was fetched: the same rows, the same bits
        assert n3 == BATCH and sums3.tobytes() == sums.tobytes()
    finally:
        eng.close()
        plain.close()


def test_end_to_end_equals_the_restatement_on_the_engines_own_outputs(net_file, rows):
    from p3achygo_amd import engine
    _end_to_end(net_file, rows, NET, engine.FLAG_AUX, False)


@pytest.mark.parametrize("net,flag,calibrate", [("test_b2d64h2_tfm", 0, False), (NET, "FLAG_FP32", False),
                                                ("test_b3c192classic", "FLAG_INT8", True)])
def test_other_plans(net_file, rows, net, flag, calibrate):
    from p3achygo_amd import engine
    _end_to_end(net_file, rows, net, engine.FLAG_AUX | (getattr(engine, flag) if flag else 0), calibrate)


# ---- 3. composition --------------------------------------------------------------------------------
def test_targets_on_some_slots_and_rows_that_are_not_slots(aux_engine, rows):
    eng = aux_engine
    feats, _, targets = rows
    for s in range(BATCH):
        eng.LoadBatch(s, feats[s:s + 1])
        if s % 2 == 1:
            eng.load_targets(s, targets[s:s + 1])
    eng.RunInference()
    sums, n = eng.loss()
    assert n == 4 and [eng.get_loss(s) is None for s in range(BATCH)] == [True, False] * 4
    terms = _check_slots(eng, [1, 3, 5, 7], targets[[1, 3, 5, 7]], "odd slots")
    _check_sums(sums, terms)
    # fetch two slots, load two others anew: the next run has six rows, rows != slots
    eng.GetBatch(0), eng.GetBatch(3)
    eng.LoadBatch(5, feats[2:3]); eng.load_targets(5, targets[2:3])
    eng.LoadBatch(6, feats[0:1]); eng.load_targets(6, targets[0:1])
    eng.RunInference()
    sums, n = eng.loss()
    assert n == 4 and eng.get_loss(3) is None and eng.get_loss(0) is None      # 1, 5, 6, 7 have targets
    terms = _check_slots(eng, [1, 5, 6, 7], targets[[1, 2, 0, 7]], "compacted")
    _check_sums(sums, terms)
    # a slot loaded again after the run is left out, with or without new targets
    eng.LoadBatch(7, feats[4:5]); eng.load_targets(7, targets[4:5])
    eng.LoadBatch(1, feats[1:2])
    sums, n = eng.loss()
    assert n == 2 and eng.get_loss(7) is None and eng.get_loss(1) is None and eng.get_loss(5) is not None
    # the test hook ends the run's scoring
    from p3achygo_amd import engine
    raw, aux, tg = lr.synthetic(engine.targets_dtype(), 2)
    eng.debug_loss_rows(raw, aux, tg)
    assert eng.loss()[1] == 0 and eng.get_loss(5) is None and eng.score()[1] == 0
    for s in range(BATCH):                               # leave the shared engine with nothing pending
        eng.LoadBatch(s, feats[s:s + 1])
    eng.RunInference()
    for s in range(BATCH):
        eng.GetBatch(s)


def test_run_all_slots_leaves_slots_without_targets_out(built, weight_files, rows):
    from p3achygo_amd import engine
    feats, _, targets = rows
    eng = engine.HipEngine(weight_files(NET), BATCH, flags=engine.FLAG_AUX | engine.FLAG_RUN_ALL_SLOTS)
    try:
        for s in (2, 5):
            eng.LoadBatch(s, feats[s:s + 1])
            eng.load_targets(s, targets[s:s + 1])
        eng.load_targets(6, targets[6:7])
        eng.LoadBatch(6, feats[6:7])                       # a new load clears the targets given before it
        eng.RunInference()
        sums, n = eng.loss()
        assert n == 2 and eng.get_loss(6) is None and eng.get_loss(0) is None
        _check_sums(sums, _check_slots(eng, [2, 5], targets[[2, 5]], "run all slots"))
    finally:
        eng.close()


def test_an_engine_without_the_aux_flag_refuses_by_name(built, weight_files, rows):
    from p3achygo_amd import engine
    feats, _, targets = rows
    eng = engine.HipEngine(weight_files(NET), BATCH)
    try:
        eng.LoadBatch(0, feats[0:1])
        eng.load_targets(0, targets[0:1])                  # accepted
        eng.RunInference()
        with pytest.raises(engine.EngineError, match="P3HIP_FLAG_AUX"):
            eng.loss()
        raw, aux, tg = lr.synthetic(engine.targets_dtype(), 1)
        with pytest.raises(engine.EngineError, match="P3HIP_FLAG_AUX"):
            eng.debug_loss_rows(raw, aux, tg)
        assert eng.get_loss(0) is None
    finally:
        eng.close()


# ---- 5. loss_chunks ----------------------------------------------------------------------------------
def test_loss_chunks_equals_val_on_the_engines_fetched_outputs(built, weight_files):
    from p3achygo_amd import dataset, engine
    eng = engine.HipEngine(weight_files(NET), 4, flags=engine.FLAG_AUX)
    try:
        ds = dataset.Dataset(dc.FIXTURE)
        per_batch, bnd = [], []
        prev = 0
        for lo in (0, 4):                                  # two batches, the second short
            f, t = ds.features[lo:lo + 4], ds.targets[lo:lo + 4]
            prev = dataset.load_batch(eng, f, None, prev)
            eng.RunInference()
            raw = np.stack([eng.get_raw(s) for s in range(len(f))])
            aux = np.stack([eng.GetAux(s) for s in range(len(f))])
            want, bound, _ = lr.bounds(raw, aux, t)
            per_batch.append(want)
            bnd.append(bound)
        dataset.release(eng, 0, prev)
        for mine, theirs in ((dataset.LossCoeffs.rl(), lr.RL), (dataset.LossCoeffs.sl(), lr.SL)):
            got = dataset.loss_chunks(eng, [dc.FIXTURE], mine)
            want = lr.val(per_batch, theirs)
            # every loss is a weighted mean of terms that each lie within their bound: the bounds combine the same way
            slack = lr.val(bnd, {k: abs(v) for k, v in theirs.items()})
            assert got["batches"] == 2 and got["positions"] == 6
            for k in lr.LOSSES:
                print(f"{k:18s} {got[k]:.9g} want {want[k]:.9g} bound {slack[k]:.3g}")
                assert abs(got[k] - want[k]) <= slack[k], (k, got[k], want[k], slack[k])
            assert got["move_accuracy"] == want["move_accuracy"] and got["outcome_accuracy"] == want["outcome_accuracy"]
            assert got["loss"] > 0 and got["policy"] > 0
        assert dataset.loss_chunks(eng, [dc.FIXTURE], dataset.LossCoeffs.rl(), max_batches=1)["positions"] == 4
    finally:
        eng.close()


# ---- the tools ---------------------------------------------------------------------------------------
def test_tools_print_the_losses_and_the_ab_agrees(built, weight_files, tmp_path, capsys):
    """tools/dataset_benchmark.py --loss on the fixture chunk (the block val() logs, and "val" in the JSON line) and
    tools/gpu_loss_ab.py at a small size: both legs return the same sums."""
    import importlib.util
    import json

    def load(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(dc.ROOT, "tools", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    out, ab = str(tmp_path / "bench.jsonl"), str(tmp_path / "ab.jsonl")
    load("dataset_benchmark").main([weight_files(NET), dc.FIXTURE, "--batch", "4", "--warmup", "1", "--out", out, "--loss", "rl"])
    text = capsys.readouterr().out
    assert "Validation losses (rl coefficients, 6 positions, 2 batches" in text
    for name in lr.LOSSES + ("move accuracy", "outcome accuracy"):
        assert f"  {name}: " in text, name
    (rec,) = [json.loads(l) for l in open(out)]
    assert rec["flags"] & 1024 and rec["val"]["positions"] == 6 and rec["val"]["coeffs"] == "rl" and rec["val"]["loss"] > 0
    assert rec["stats"]["num_examples"] == 6                                   # the scoring block is still there
    load("gpu_loss_ab").main([weight_files(NET), "--batch", "16", "--games", "4", "--reps", "1", "--warmup", "1", "--out", ab])
    (rec,) = [json.loads(l) for l in open(ab)]
    assert rec["sums_agree"] and rec["positions"] == 32 and rec["batches"] == 2
    assert rec["p3hip_loss_us_per_batch"] > 0 and rec["device_positions_per_s"] > 0 and rec["host_positions_per_s"] > 0
