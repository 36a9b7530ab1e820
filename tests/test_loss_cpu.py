"""The validation losses without a GPU: the numpy restatement (tests/loss_restatement.py) pinned by answers derived by
hand, the reader's targets (p3achygo_amd/host/tf_reader.h ParseTargets behind p3host_dataset_targets,
dataset.Dataset.targets) against a Python parse of the same bytes, dataset.loss_from_sums against the restatement's batch
function, and the layout of p3hip_targets in the header, in numpy and in the reader."""
import os
import re
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dataset_common as dc  # noqa: E402
import loss_restatement as lr  # noqa: E402

TARGET_FIELDS = ("policy", "policy_aux_dist", "own", "mcts_value_dist", "score_margin", "q6", "q16", "q50", "q6_score",
                 "q16_score", "q50_score", "policy_aux", "has_pi_aux_dist", "has_mcts_value_dist")


@pytest.fixture(scope="module")
def mods(built):
    from p3achygo_amd import dataset, engine
    return dataset, engine


def _blank():
    """All-zero predictions and a target with a one-hot policy on move 5; everything else zero."""
    tg = {f: 0 for f in TARGET_FIELDS}
    tg["policy"] = np.zeros(362, np.float32)
    tg["policy"][5] = 1
    tg["policy_aux_dist"], tg["own"], tg["mcts_value_dist"] = np.zeros(362, np.float32), np.zeros(361, np.float32), np.zeros(51, np.float32)
    return np.zeros(lr.RAW_LEN, np.float32), np.zeros(lr.AUX_LEN, np.float32), tg


# ---- known answers ---------------------------------------------------------------------------------
def test_known_answers_of_the_restatement(mods):
    assert mods[1].LOSS_TERMS == lr.TERMS              # the terms the engine computes, in its order
    raw, aux, tg = _blank()
    t = lr.terms(raw, aux, tg)
    # uniform softmax 1/362 against a one-hot: 1 log(362) for the hot entry, and the 361 zeros clipped to 1e-7
    want0 = np.log(362.0) + 361 * 1e-7 * np.log(362e-7)
    assert t[0] == pytest.approx(want0, rel=1e-6) and t[15] == pytest.approx(want0 * lr.optimistic_weight([0] * 3, [0] * 3, [0] * 3, np.float64), rel=1e-6)
    assert t[3] == pytest.approx(np.log(2.0), rel=1e-12)                 # margin 0: g = [.5, .5] on equal logits
    assert t[2] == pytest.approx(np.log(362.0), rel=1e-12) and t[1] == 0  # no distribution: the scalar term, on move 0
    assert t[7] == pytest.approx(np.log(800.0), rel=1e-12)
    # cdf of a uniform softmax against a step at k = 400: sum_{j<400} ((j+1)/800)^2 + sum_{j>=400} (1 - (j+1)/800)^2
    j = np.arange(800)
    assert t[8] == pytest.approx((np.where(j >= 400, 1.0, 0.0) - (j + 1) / 800.0) ** 2 @ np.ones(800), rel=1e-12)
    assert t[16] == 0 and t[9] == 0 and t[10] == 0 and (t[4:7] == 0).all() and (t[11:14] == 0).all()
    # soft target: the one-hot stays one-hot under ^0.25
    assert t[14] == pytest.approx(want0, rel=1e-6)
    assert t[17] == 0 and t[18] == 0     # argmax of equal logits is move 0, the label is 5; argmax(outcome) = 0 but margin >= 0

    # the score bin: floor, not truncation, and the clamp
    assert [lr.score_index(m) for m in (-1000.0, 1000.0, -0.5, 0.0, 0.5, -1.0, 399.0, 398.99, -400.0, -400.5)] == \
        [0, 799, 399, 400, 400, 399, 799, 798, 0, 0]
    for margin, k in ((-1000.0, 0), (1000.0, 799), (-0.5, 399)):
        raw, aux, tg = _blank()
        raw[726 + k] = 3.0
        tg["score_margin"] = margin
        t = lr.terms(raw, aux, tg)
        assert t[7] == pytest.approx(np.log(799.0 + np.exp(3.0)) - 3.0, rel=1e-12), (margin, k)
        g = (0.0, 1.0) if margin > 0 else (1.0, 0.0)
        assert t[3] == pytest.approx(np.log(2.0), rel=1e-12) and t[18] == float(margin < 0)

    # outcome: g picks the logit of the side that won
    raw, aux, tg = _blank()
    raw[724:726] = (1.0, 3.0)
    tg["score_margin"] = 2.5
    assert lr.terms(raw, aux, tg)[3] == pytest.approx(np.log1p(np.exp(-2.0)), rel=1e-12)
    tg["score_margin"] = -2.5
    t = lr.terms(raw, aux, tg)
    assert t[3] == pytest.approx(2.0 + np.log1p(np.exp(-2.0)), rel=1e-12) and t[18] == 0

    # Huber on both sides of delta = 1, and error = y_pred - y_true
    assert lr.huber(0.0, 0.3, np.float64) == pytest.approx(0.045) and lr.huber(0.3, 0.0, np.float64) == pytest.approx(0.045)
    assert lr.huber(0.0, 30.0, np.float64) == 29.5 and lr.huber(1.0, 0.0, np.float64) == 0.5
    raw, aux, tg = _blank()
    aux[729:732] = (3.0, 300.0, 0.0)                  # q_score predictions against targets of 0: residuals 0.3, 30, 0
    aux[724:727] = (0.5, 0.0, 0.0)                    # q6 prediction 0.5 against 0: a squared error of 0.25
    raw[1887] = 4.0                                   # ... judged by a q6_err of 4: residual 3.75
    t = lr.terms(raw, aux, tg)
    assert t[12] == pytest.approx((0.045 + 29.5 + 0.0) / 3) and t[4] == 0.25
    assert t[11] == pytest.approx((3.25 + 0 + 0) / 3)
    assert t[13] == pytest.approx((0.5 * 0.09 ** 2 + (900.0 - 0.5) + 0) / 3)

    # mcts: has = 1 with all counts zero: the total becomes 1, the target all zeros, every entry at the clip
    raw, aux, tg = _blank()
    tg["has_mcts_value_dist"] = 1
    assert lr.terms(raw, aux, tg)[16] == pytest.approx(51 * 1e-7 * np.log(51e-7), rel=1e-6)
    tg["mcts_value_dist"][7] = 1 << 20
    assert lr.terms(raw, aux, tg)[16] == pytest.approx(np.log(51.0) + 50 * 1e-7 * np.log(51e-7), rel=1e-6)
    tg["has_mcts_value_dist"] = 0
    assert lr.terms(raw, aux, tg)[16] == 0

    # policy_aux = 361 is the pass entry; the distribution term replaces the scalar one when there is one
    raw, aux, tg = _blank()
    aux[361] = 2.0
    tg["policy_aux"] = 361
    assert lr.terms(raw, aux, tg)[2] == pytest.approx(np.log(361.0 + np.exp(2.0)) - 2.0, rel=1e-12)
    aux[361] = -80.0
    assert lr.terms(raw, aux, tg)[2] == 50.0                              # the clip
    tg["has_pi_aux_dist"] = 1
    tg["policy_aux_dist"][361] = 1
    t = lr.terms(raw, aux, tg)
    assert t[2] == 0 and t[1] == pytest.approx(np.log(1 / 1e-7) + 361 * 1e-7 * np.log(1e-7 * 361.0), rel=1e-5)

    # the optimistic weight: z = 4/7 (3 z6 + 1.5 z16 + .75 z50) / 3 with z_h = (q - q_pred) / sqrt(err + 1e-6)
    w = lr.optimistic_weight([0.5, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], np.float64)
    z = 4.0 / 7.0 * 3 * (0.5 / np.sqrt(1.0 + 1e-6)) / 3
    assert w == pytest.approx(1 / (1 + np.exp(-3 * (z - 1))), rel=1e-7)
    assert lr.optimistic_weight([0.9] * 3, [0.0] * 3, [0.0] * 3, np.float64) > 0.9999
    assert lr.optimistic_weight([-0.9] * 3, [0.0] * 3, [0.0] * 3, np.float64) < 1e-4

    # the float32 twin stays close to the checker and is float32 all the way
    raw, aux, tg = _blank()
    raw[:] = np.random.default_rng(0).normal(0, 1, lr.RAW_LEN)
    aux[:] = np.abs(np.random.default_rng(1).normal(0, 1, lr.AUX_LEN))
    a, b = lr.terms(raw, aux, tg), lr.terms(raw, aux, tg, np.float32)
    assert b.dtype == np.float32 and np.abs(a - b).max() < 1e-4 * max(1, np.abs(a).max()) and np.abs(a - b).max() > 0


def test_synthetic_rows_take_every_branch(mods):
    _, engine = mods
    raw, aux, tg = lr.synthetic(engine.targets_dtype(), 8)
    want = lr.terms_rows(raw, aux, tg)
    assert np.isfinite(want).all()
    for vec in (raw[0, 0:362], raw[0, 362:724], aux[0, 0:362], aux[0, 362:724]):       # peaked to 0.999, both sides of the clip
        p = lr.softmax(vec, np.float64)
        assert p.max() == pytest.approx(0.999, rel=1e-4) and (p < 1e-7).sum() > 20 and ((p > 1e-7) & (p < 1e-3)).sum() > 20
    assert (tg["policy"][0] < 1e-7).sum() > 20 and tg["policy"][0].max() == pytest.approx(0.999, rel=1e-4)
    assert np.abs(raw[:, 726:1526]).max() > 9.9 and np.abs(raw[:, 1526:1887]).max() == np.float32(0.9999)
    assert {0.0, 0.5, -0.5, 1000.0, -1000.0} <= set(tg["score_margin"].tolist())
    assert set(tg["has_pi_aux_dist"]) == {0, 1} == set(tg["has_mcts_value_dist"]) and {0, 360, 361} <= set(tg["policy_aux"].tolist())
    q = np.stack([tg["q6"], tg["q16"], tg["q50"]], 1)
    err = np.concatenate([raw[:, 1887:1888], aux[:, 727:729]], 1)
    w = [lr.optimistic_weight(q[i], aux[i, 724:727], err[i], np.float64) for i in range(8)]
    assert (err[0] == 0).all() and (err[2] == 4).all() and min(w) < 1e-4 and max(w) > 0.9999 and any(1e-4 < v < 0.9999 for v in w)
    assert tg["mcts_value_dist"][0].sum() == 0 and tg["has_mcts_value_dist"][0] == 1 and tg["mcts_value_dist"][1].sum() == 1 << 20
    assert want[2, 12] == pytest.approx(0.045) and want[3, 12] == pytest.approx(29.5)      # Huber residuals 0.3 and 30
    assert set(want[:, 17]) == {0.0, 1.0} == set(want[:, 18])
    top2 = np.sort(raw[:, 0:362], axis=1)[:, -2:]
    gap = top2[:, 1] - top2[:, 0]
    assert (np.delete(gap, 4) >= 1e-3).all() and gap[4] == 0 and want[4, 17] == 1          # the one deliberate tie: lower index
    assert (np.abs(raw[:, 724] - raw[:, 725]) >= 1e-3).all()


# ---- the reader ------------------------------------------------------------------------------------
def _assert_targets_equal(got, want, where):
    for f in TARGET_FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f], np.asarray(got[f]).dtype)
        assert g.tobytes() == w.tobytes(), (where, f, g, w)


def test_fixture_targets_equal_a_python_parse(mods):
    dataset, engine = mods
    ds = dataset.Dataset(dc.FIXTURE)
    assert dataset.Chunk is dataset.Dataset and ds.targets.dtype == engine.targets_dtype()
    assert ds.has_targets.tolist() == [True] * 6
    assert ds.targets["has_pi_aux_dist"].tolist() == [0, 0, 0, 1, 1, 1] == ds.targets["has_mcts_value_dist"].tolist()
    pay = lr.payloads(open(dc.FIXTURE, "rb").read())
    for i in range(6):
        want = lr.targets_from_example(lr.parse_example(pay[i]))
        assert want is not None
        _assert_targets_equal(ds.targets[i], want, i)
        assert ds.targets["policy"][i].tobytes() == ds.labels["policy"][i].tobytes()
        assert ds.targets["score_margin"][i] == ds.labels["score_margin"][i]
    assert not ds.targets["policy_aux_dist"][:3].any() and not ds.targets["mcts_value_dist"][:3].any()
    assert (ds.targets["policy_aux_dist"][3:].sum(axis=1) > 0.99).all() and (ds.targets["mcts_value_dist"][3:].sum(axis=1) > 0).all()


def _target_features(color=1, own=None, pi_aux=17, **over):
    own = np.arange(361) % 3 - 1 if own is None else own
    f = dict(dc.base_features(color=color), own=dc.bytes_feature(np.asarray(own, np.int8).tobytes()),
             pi_aux=dc.bytes_feature(np.int16(pi_aux).tobytes()))
    for k, v in (("q6", 0.25), ("q16", -0.5), ("q50", 0.75), ("q6_score", 3.5), ("q16_score", -12.25), ("q50_score", 40.0)):
        f[k] = dc.float_feature(v)
    f.update(over)
    return {k: v for k, v in f.items() if v is not None}


def test_targets_of_hand_built_records(mods, tmp_path):
    """own negated for white; the optional keys absent, empty or present; records the trainer's parse would refuse load
    without targets and with their labels intact."""
    dataset, _ = mods
    own = (np.arange(361) % 3 - 1).astype(np.int8)
    dist = np.random.default_rng(3).random(362).astype(np.float32)
    counts = np.arange(51, dtype=np.uint32) * 1000
    counts[50] = 0x7FFFFFFF
    empty_list = dc.ld(1, b"")                                # a bytes_list with no value: `.values` is empty
    recs = [
        _target_features(color=1),                                                          # 0 black
        _target_features(color=-1),                                                         # 1 white: own negated
        _target_features(pi_aux_dist=dc.bytes_feature(dist.tobytes()), mcts_value_dist=dc.bytes_feature(counts.tobytes())),
        _target_features(pi_aux_dist=empty_list, mcts_value_dist=empty_list, pi_aux=361),   # 3 empty: as absent
        _target_features(own=own[:360]),                                                    # 4 own one byte short
        _target_features(pi_aux=400),                                                       # 5 not a move
        _target_features(q16=None),                                                         # 6 a FixedLenFeature missing
        _target_features(pi_aux_dist=dc.bytes_feature(dist.tobytes()[:-4])),                # 7 a short distribution
        _target_features(q6=dc.bytes_feature(b"abcd")),                                     # 8 the wrong kind
        _target_features(pi_aux=-1),                                                        # 9 the old recorder's "none"
        _target_features(mcts_value_dist=dc.float_feature(1.0)),                            # 10 the wrong kind, optional key
    ]
    p = tmp_path / "targets.tfrecord"
    p.write_bytes(b"".join(dc.frame(dc.example(r, junk=i % 2 == 1)) for i, r in enumerate(recs)))
    ds = dataset.Dataset(str(p))
    assert len(ds) == len(recs)
    assert ds.has_targets.tolist() == [True, True, True, True] + [False] * 7
    t = ds.targets
    assert t["own"][0].tobytes() == own.astype(np.float32).tobytes() and t["own"][1].tobytes() == (-own.astype(np.int32)).astype(np.float32).tobytes()     # negated as int32: no -0.0
    assert t["policy_aux_dist"][2].tobytes() == dist.tobytes() and t["has_pi_aux_dist"].tolist()[:4] == [0, 0, 1, 0]
    assert t["mcts_value_dist"][2].tobytes() == counts.astype(np.int32).astype(np.float32).tobytes()
    assert t["has_mcts_value_dist"].tolist()[:4] == [0, 0, 1, 0] and t["policy_aux"].tolist()[:4] == [17, 17, 17, 361]
    assert (t["q6"][:4], t["q16"][0], t["q50"][0], t["q6_score"][0], t["q16_score"][0], t["q50_score"][0]) == \
        (pytest.approx([0.25] * 4), -0.5, 0.75, 3.5, -12.25, 40.0)
    for i, r in enumerate(recs):
        want = lr.targets_from_example(lr.parse_example(dc.example(r)))
        assert (want is not None) == bool(ds.has_targets[i]), i
        if want is not None:
            _assert_targets_equal(t[i], want, i)
        else:
            assert not t[i].tobytes().strip(b"\0"), i                                        # zeros where there are none
        assert ds.labels["policy"][i][5] == 1 and ds.labels["score_margin"][i] == 1.5 and ds.labels["did_win"][i] == 1
        assert i == 1 or ds.features[i].tobytes() == ds.features[0].tobytes()                 # the rows load alike
    # batches hands the targets over with the rows
    got = list(dataset.batches([str(p)], 4, with_targets=True))
    assert [len(b[2]) for b in got] == [4, 4, 3] and got[1][3].tolist() == [False] * 4
    assert got[0][2].tobytes() == t[:4].tobytes()


def test_target_parsing_under_address_and_ub_sanitizers(mods, tmp_path):
    """tests/native/dataset_targets_main.cc over the fixture and over records whose target keys have every wrong length
    and kind, built with -fsanitize=address,undefined (runtimes linked statically) and run as a child process; it must
    count the rows and targets the library counts."""
    dataset, _ = mods
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the reader's sanitizer program"
    def _with(**feature):
        return dict(_target_features(), **feature)

    recs = [_target_features()]
    for key, n in (("own", 361), ("pi_aux", 2), ("pi_aux_dist", 1448), ("mcts_value_dist", 204)):
        for m in sorted({0, 1, n - 1, n + 1, 2 * n}):
            recs.append(_with(**{key: dc.bytes_feature(bytes(m))}))
        recs.append(_with(**{key: dc.float_feature(2.0)}))
        recs.append(_with(**{key: dc.ld(1, b"")}))                               # an empty bytes_list
        recs.append(_with(**{key: dc.ld(1, b"\x0a\x7f")}))                        # a value that overruns its list
        recs.append(_with(**{key: dc.ld(1, dc.ld(1, bytes(n)) + dc.ld(1, bytes(3)))}))   # two values
    for key in ("q6", "q50_score"):
        recs += [_with(**{key: dc.bytes_feature(b"abcd")}), _with(**{key: dc.ld(2, dc.ld(1, bytes(8)))}),
                 _with(**{key: dc.ld(2, dc.ld(1, bytes(3)))}), _with(**{key: dc.ld(2, b"")})]
    p = tmp_path / "lengths.tfrecord"
    p.write_bytes(b"".join(dc.frame(dc.example(r, junk=i % 3 == 0)) for i, r in enumerate(recs)))
    ds = dataset.Dataset(str(p))
    assert len(ds) == len(recs) and ds.has_targets[0] and 0 < ds.has_targets.sum() < len(recs) // 2
    for i, r in enumerate(recs):                                                           # and the Python parse agrees
        assert (lr.targets_of_payload(dc.example(r)) is not None) == bool(ds.has_targets[i]), i
    exe = tmp_path / "dataset_targets_main"
    src = os.path.join(dc.ROOT, "tests", "native", "dataset_targets_main.cc")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", src, "-o", str(exe), "-lz"], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), dc.FIXTURE, str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert "rows 6 targets 6" in lines[0] and f"rows {len(recs)} targets {int(ds.has_targets.sum())}" in lines[1], r.stdout


def test_host_loss_terms_equal_the_restatement(mods):
    dataset, engine = mods
    raw, aux, tg = lr.synthetic(engine.targets_dtype(), 16)
    got, want = dataset.host_loss_terms(raw, aux, tg), lr.terms_rows(raw, aux, tg)
    assert got.shape == (16, 19) and (got[:, 17:] == want[:, 17:]).all()
    assert (np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all()


def test_recorded_chunk_round_trips_every_target_field(mods, tmp_path):
    """A chunk the host's recorder wrote: every row has targets, and each field equals a Python parse of the inflated
    bytes bit for bit; the value distribution and the policy given to the recorder come back as they went in."""
    dataset, _ = mods
    n = len(dc.GAME)
    rng = np.random.default_rng(9)
    vdist = rng.integers(0, 5000, (n, 51)).astype(np.uint32)
    lib = dc.recorder_lib()
    h = lib.p3host_tfrec_new(str(tmp_path).encode(), 0, b"ds")
    mv, pi = np.asarray(dc.GAME, np.int32), dc.game_pi()
    q = rng.uniform(0.2, 0.8, n).astype(np.float32)
    score = rng.normal(0, 8, n).astype(np.float32)
    assert lib.p3host_tfrec_record(h, mv.ctypes.data, n, dc.KOMI, pi.ctypes.data, None, q.ctypes.data, score.ctypes.data, None,
                                   vdist.ctypes.data, None) == 0
    assert lib.p3host_tfrec_flush(h) == n
    lib.p3host_tfrec_free(h)
    (path,) = [os.path.join(tmp_path, f) for f in os.listdir(tmp_path) if f.endswith(".tfrecord.zz")]
    ds = dataset.Dataset(path)
    assert len(ds) == n and ds.has_targets.all()
    pay = lr.payloads(zlib.decompress(open(path, "rb").read()))
    colors = set()
    for i in range(n):
        ex = lr.parse_example(pay[i])
        want = lr.targets_from_example(ex)
        _assert_targets_equal(ds.targets[i], want, i)
        color = int(np.frombuffer(ex["color"][1][0], np.int8)[0])
        colors.add(color)
        own = np.frombuffer(ex["own"][1][0], np.int8).astype(np.int32)
        assert ds.targets["own"][i].tobytes() == (own if color == 1 else -own).astype(np.float32).tobytes()
        assert ds.targets["policy"][i].tobytes() == pi[i].tobytes()
        assert ds.targets["mcts_value_dist"][i].tobytes() == vdist[i].astype(np.float32).tobytes() and ds.targets["has_mcts_value_dist"][i] == 1
    assert colors == {1, -1} and np.abs(ds.targets["own"]).sum() > 0
    assert len(set(ds.targets["q6"].tolist())) > 1 and len(set(ds.targets["q6_score"].tolist())) > 1
    assert (ds.targets["policy_aux"] >= 0).all() and (ds.targets["policy_aux"] <= 361).all()


def test_targets_of_a_bad_row_index(mods):
    _, engine = mods
    from p3achygo_amd import host_api
    h = host_api.dataset_open(dc.FIXTURE)
    try:
        buf = np.full(engine.targets_dtype().itemsize, 0x5A, np.uint8)
        for i in (-1, 6, 1 << 40):
            with pytest.raises(IndexError):
                host_api.dataset_targets(h, i, buf.ctypes.data)
        assert (buf == 0x5A).all()
        assert host_api.dataset_targets(h, 5, buf.ctypes.data) and buf.view(engine.targets_dtype())["policy_aux"][0] == 361
    finally:
        host_api.dataset_close(h)


# ---- loss_from_sums --------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_loss_from_sums_equals_the_restatements_batch_function(mods, seed):
    dataset, engine = mods
    assert engine.LOSS_TERMS == lr.TERMS and dataset.LOSS_NAMES == lr.LOSSES and engine.NUM_LOSS_TERMS == 19
    rng = np.random.default_rng(seed)
    n = (5, 64, 1)[seed]
    T = np.abs(rng.normal(0, 2, (n, 19))).astype(np.float32)
    if seed == 1:                                   # both batch-level clips bite: means above 200 and above 1000
        T[:, 12] += 250
        T[:, 13] += 1500
    T[:, 17:] = rng.integers(0, 2, (n, 2))
    sums = T.astype(np.float64).sum(axis=0)
    for mine, theirs in ((dataset.LossCoeffs.rl(), lr.RL), (dataset.LossCoeffs.sl(), lr.SL)):
        import dataclasses
        assert {k: float(v) for k, v in dataclasses.asdict(mine).items()} == {k: float(v) for k, v in theirs.items()}
        got, want = dataset.loss_from_sums(sums, n, mine), lr.batch_losses(T, theirs)
        assert tuple(got) == lr.LOSSES
        for k in lr.LOSSES:
            assert got[k] == pytest.approx(want[k], rel=1e-12, abs=1e-15), k
        if seed == 1:
            assert got["q_score"] == 200.0 and got["q_score_err"] == 1000.0
        else:
            assert got["q_score"] < 200.0 and got["q_score_err"] < 1000.0
    # the weighted total by hand on unit means: every loss 1 (gamma_sq too)
    one = dataset.loss_from_sums(np.ones(19), 1, dataset.LossCoeffs.rl())
    assert one["loss"] == pytest.approx(1.0 + 0.15 + 0.15 * 0.6 + (1.5 + 0.7 + 0.4 + 0.3 + 0.02 + 0.45) + 0.02 + 0.005 + 0.125 +
                                        3.0 + 0.2 + 0.2 + 4.0 + 1.0, rel=1e-12)


# ---- the struct ------------------------------------------------------------------------------------
def test_struct_layout_agrees_between_header_numpy_and_reader(mods, tmp_path):
    dataset, engine = mods
    dt = engine.targets_dtype()
    assert dt.itemsize == 4 * 1146 and dt.names == TARGET_FIELDS
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed to read the header's layout"
    header = os.path.join(dc.ROOT, "include", "p3hip.h")
    lines = "".join(f'  printf("{f} %zu\\n", offsetof(p3hip_targets, {f}));\n' for f in TARGET_FIELDS)
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "{header}"\nint main(void) {{\n{lines}'
                   '  printf("sizeof %zu\\n", sizeof(p3hip_targets));\n  printf("terms %d\\n", P3HIP_NUM_LOSS_TERMS);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == dt.itemsize and int(out["terms"]) == engine.NUM_LOSS_TERMS == len(engine.LOSS_TERMS)
    for f in TARGET_FIELDS:
        assert int(out[f]) == dt.fields[f][1], f
    # the header's table of terms names them in LOSS_TERMS' order
    text = open(header).read()
    named = re.findall(r"^ \*   \[(\d+)(?:\.\.\d+)?\]\s+(\w+)", text[text.index("The 19 terms of one position"):], re.M)
    assert [n for _, n in named[:17]] == ["policy", "policy_aux_dist", "policy_aux_scalar", "outcome", "q6", "score_pdf",
                                          "score_cdf", "own", "gamma_sq", "q_err", "q_score", "q_score_err", "pi_soft",
                                          "pi_optimistic", "mcts_dist", "move_hit", "outcome_hit"]
    assert [int(i) for i, _ in named[:17]] == [0, 1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18]
    # the reader fills the same layout: the fixture's last row through the numpy view
    ds = dataset.Dataset(dc.FIXTURE)
    want = lr.targets_from_example(lr.parse_example(lr.payloads(open(dc.FIXTURE, "rb").read())[5]))
    _assert_targets_equal(ds.targets[5], want, 5)
    for name in ("p3hip_load_targets", "p3hip_loss", "p3hip_get_loss", "p3hip_debug_loss_rows"):
        assert name in engine.EXPORTS and re.search(rf"\b{name}\(", text)
