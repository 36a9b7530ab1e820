"""Chunk reader of the host (p3achygo_amd/host/tf_reader.h behind p3host_dataset_*, p3achygo_amd/dataset.py) and the
numpy restatement of the scoring terms (tests/dataset_restatement.py).  No GPU.

The fixture tests/golden/dataset/mixed_schema.tfrecord is the reference's python/test_data/mixed_schema.tfrecord, the one
chunk there that TensorFlow itself wrote: six plain-TFRecord records, three of the old schema (no pi_aux_dist /
mcts_value_dist) and three of the new one."""
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dataset_common as dc  # noqa: E402
import dataset_restatement as dr  # noqa: E402


@pytest.fixture(scope="module")
def ds_mod(built):
    from p3achygo_amd import dataset
    return dataset


@pytest.fixture(scope="module")
def fixture_bytes():
    raw = open(dc.FIXTURE, "rb").read()
    assert len(raw) == 29436 and len(raw) == sum(16 + n for n in dc.FIXTURE_PAYLOADS)
    return raw


def _open_error(ds_mod, tmp_path, name, data, mode=0):
    from p3achygo_amd import host_api
    p = tmp_path / name
    p.write_bytes(data)
    with pytest.raises(host_api.DatasetError) as ei:
        ds_mod.Dataset(str(p), mode)
    return str(ei.value)


# ---- the fixture ---------------------------------------------------------------------------------
def test_fixture_rows(ds_mod, fixture_bytes):
    offs = dc.record_offsets(fixture_bytes)
    assert tuple(struct.unpack_from("<Q", fixture_bytes, o)[0] for o in offs) == dc.FIXTURE_PAYLOADS
    ds = ds_mod.Dataset(dc.FIXTURE)
    assert len(ds) == 6
    f, l = ds.features, ds.labels
    assert list(l["score_margin"]) == [5.5, -5.5, 0.5, 3.5, -3.5, 0.0]
    assert list(l["did_win"]) == [1, 0, 1, 1, 0, 1]
    assert list(f["komi"]) == [6.5] * 6 and list(f["bsize"]) == [19] * 6
    assert list(f["color"]) == [1, -1, 1, 1, -1, 1]
    for grid in ("board", "stones_atari", "stones_two_liberties", "stones_three_liberties", "stones_laddered"):
        assert not f[grid].any(), grid
    want_pi = np.zeros(362, np.float32)
    want_pi[0] = 1
    for i in range(6):
        assert np.array_equal(l["policy"][i], want_pi)
        # the chunk stores -1 five times: AsLoc's truncating / and % give {0,-1}, neither noop nor pass
        assert [(int(m["i"]), int(m["j"])) for m in f["last_moves"][i]] == [(0, -1)] * 5
    # the new-schema records (3..5) load like the old ones: same fields, nothing else differs but the labels
    assert f[3].tobytes() == f[0].tobytes() and f[4].tobytes() == f[1].tobytes()


def test_fixture_modes_and_zlib(ds_mod, fixture_bytes, tmp_path):
    from p3achygo_amd import host_api
    plain = ds_mod.Dataset(dc.FIXTURE, host_api.DATASET_PLAIN)
    z = tmp_path / "fixture.tfrecord.zz"
    z.write_bytes(zlib.compress(fixture_bytes, 2))
    for mode in (host_api.DATASET_AUTO, host_api.DATASET_ZLIB):
        ds = ds_mod.Dataset(str(z), mode)
        assert ds.features.tobytes() == plain.features.tobytes() and ds.labels.tobytes() == plain.labels.tobytes()
    assert "record 0" in _open_error(ds_mod, tmp_path, "as_plain", z.read_bytes(), host_api.DATASET_PLAIN)
    with pytest.raises(host_api.DatasetError, match="cannot open"):
        ds_mod.Dataset(str(tmp_path / "nothing_here"))
    # a plain record of 376 bytes starts 78 01, which is a zlib header too: the length CRC decides
    odd = dc.frame(b"\x00" * 376)
    assert odd[:2] == b"\x78\x01"
    msg = _open_error(ds_mod, tmp_path, "odd", odd)
    assert msg.startswith("record 0:") and "tf.Example" in msg and "zlib" not in msg


def test_last_move_decoding_and_wire_variants(ds_mod, tmp_path):
    """361 -> pass {19,0}, the recorder's noop -20 -> {-1,-1}, -1 -> {0,-1}, 360 -> {18,18}; floats packed or not,
    unknown fields of every wire type, values in front of keys, keys in any order: the same row."""
    feats = dc.base_features(color=-1, margin=-0.0, komi=0.5, last=(-20, -1, 361, 3, 360), hot=361)
    plain = dict(feats, score_margin=dc.float_feature(-0.0, packed=False), komi=dc.float_feature(0.5, packed=False))
    extra = dict(feats, own=dc.bytes_feature(bytes(361)), q6=dc.float_feature(0.25), pi_aux_dist=dc.bytes_feature(bytes(1448)),
                 visits=dc.ld(3, dc.ld(1, dc.varint(7) + dc.varint(9))))
    recs = [dc.example(feats), dc.example(plain, order=sorted(plain, reverse=True)), dc.example(extra, junk=True)]
    p = tmp_path / "variants.tfrecord"
    p.write_bytes(b"".join(dc.frame(r) for r in recs))
    ds = ds_mod.Dataset(str(p))
    assert len(ds) == 3
    f, l = ds.features, ds.labels
    assert [(int(m["i"]), int(m["j"])) for m in f["last_moves"][0]] == [(-1, -1), (0, -1), (19, 0), (0, 3), (18, 18)]
    assert f["color"][0] == -1 and f["komi"][0] == 0.5 and f["board"][0][3] == 1 and f["stones_three_liberties"][0][3] == 1
    assert l["did_win"][0] == 1 and np.signbit(l["score_margin"][0])      # -0.0 >= 0: a win, as in the reference
    assert l["policy"][0][361] == 1 and l["policy"][0].sum() == 1
    for i in (1, 2):
        assert f[i].tobytes() == f[0].tobytes() and l[i].tobytes() == l[0].tobytes()
    # a repeated key: the last entry wins, as in a protobuf map
    again = dc.ld(1, dc.ld(1, b"komi") + dc.ld(2, dc.float_feature(-3.5)))
    p2 = tmp_path / "twice.tfrecord"
    p2.write_bytes(dc.frame(dc.example(feats, tail=again)))
    assert ds_mod.Dataset(str(p2)).features["komi"][0] == -3.5


def test_batches_keep_a_short_last_batch(ds_mod):
    """A short last batch holds only the rows that were read (the reference pads it with default rows and scores them)."""
    got = list(ds_mod.batches([dc.FIXTURE, dc.FIXTURE], 4))
    assert [len(f) for f, _ in got] == [4, 2, 4, 2] and all(len(f) == len(l) for f, l in got)
    assert [len(f) for f, _ in ds_mod.batches([dc.FIXTURE, dc.FIXTURE], 4, max_batches=3)] == [4, 2, 4]
    assert list(got[1][1]["score_margin"]) == [-3.5, 0.0]


# ---- round trip with the recorder ----------------------------------------------------------------
def test_round_trip_with_the_recorder(ds_mod, tmp_path):
    from p3achygo_amd import host_api
    pi = dc.game_pi()
    path = dc.record_game(tmp_path)
    ds = ds_mod.Dataset(path)
    assert len(ds) == len(dc.GAME)
    want = dc.game_features()
    for m in range(len(dc.GAME)):
        assert ds.features[m].tobytes() == want[m].tobytes(), m
        assert ds.labels["policy"][m].tobytes() == pi[m].tobytes(), m
    assert [(int(x["i"]), int(x["j"])) for x in ds.features["last_moves"][4]] == [(-1, -1), (3, 3), (15, 15), (3, 15), (19, 0)]
    # the margin is the final score seen by the colour to move
    b = host_api.Board(dc.KOMI)
    for mv in dc.GAME:
        idx = abs(mv) - 1
        if idx == 361:
            b.pass_(1 if mv > 0 else -1)
        else:
            assert b.play(idx // 19, idx % 19, 1 if mv > 0 else -1)
    bs, ws, _ = b.scores()
    assert bs != ws
    for m, mv in enumerate(dc.GAME):
        margin = np.float32(bs) - np.float32(ws) if mv > 0 else np.float32(ws) - np.float32(bs)
        assert ds.labels["score_margin"][m] == margin, m
        assert ds.labels["did_win"][m] == int(margin >= 0)
    assert set(ds.labels["did_win"]) == {0, 1}


# ---- damage --------------------------------------------------------------------------------------
def test_damaged_chunks_are_refused_with_the_record_and_the_reason(ds_mod, fixture_bytes, tmp_path):
    offs = dc.record_offsets(fixture_bytes)
    raw = bytearray(fixture_bytes)
    raw[offs[3] + 12 + 1000] ^= 0x40
    msg = _open_error(ds_mod, tmp_path, "flip", bytes(raw))
    assert msg.startswith("record 3:") and "CRC" in msg and "payload" in msg

    raw = bytearray(fixture_bytes)
    struct.pack_into("<Q", raw, offs[2], 1 << 40)
    msg = _open_error(ds_mod, tmp_path, "len", bytes(raw))
    assert msg.startswith("record 2:") and "CRC" in msg and "length" in msg
    struct.pack_into("<I", raw, offs[2] + 8, dc.masked_crc(bytes(raw[offs[2]:offs[2] + 8])))
    msg = _open_error(ds_mod, tmp_path, "len_crc", bytes(raw))
    assert msg.startswith("record 2:") and "truncated" in msg and str(1 << 40) in msg

    for cut in (offs[1] + 5, offs[1] + 12, offs[1] + 2000, offs[2] - 1):
        msg = _open_error(ds_mod, tmp_path, "cut", fixture_bytes[:cut])
        assert msg.startswith("record 1:") and "truncated" in msg, (cut, msg)

    zz = zlib.compress(fixture_bytes, 2)
    for cut in (2, len(zz) // 2, len(zz) - 1):
        msg = _open_error(ds_mod, tmp_path, "zcut.zz", zz[:cut])
        assert msg.startswith("record ") and "truncated" in msg, (cut, msg)

    good = dc.base_features()
    short = dict(good, board=dc.bytes_feature(bytes(360)))
    msg = _open_error(ds_mod, tmp_path, "board", dc.frame(dc.example(good)) + dc.frame(dc.example(short)))
    assert msg.startswith("record 1:") and "wrong byte length of 'board'" in msg and "360" in msg

    no_pi = {k: v for k, v in good.items() if k != "pi"}
    msg = _open_error(ds_mod, tmp_path, "nopi", dc.frame(dc.example(good)) * 2 + dc.frame(dc.example(no_pi)))
    assert msg.startswith("record 2:") and "missing key 'pi'" in msg

    msg = _open_error(ds_mod, tmp_path, "bsize", dc.frame(dc.example(dict(good, bsize=dc.bytes_feature(bytes([9]))))))
    assert msg.startswith("record 0:") and "bsize" in msg
    msg = _open_error(ds_mod, tmp_path, "kind", dc.frame(dc.example(dict(good, komi=dc.bytes_feature(b"abcd")))))
    assert msg.startswith("record 0:") and "missing key 'komi'" in msg
    msg = _open_error(ds_mod, tmp_path, "garbage", dc.frame(b"\xff" * 40))
    assert msg.startswith("record 0:") and "tf.Example" in msg


def test_a_failed_row_read_leaves_the_outputs_untouched(built):
    import ctypes as C
    from p3achygo_amd import engine, features, host_api
    h = host_api.dataset_open(dc.FIXTURE)
    try:
        assert host_api.dataset_size(h) == 6
        f = np.full(1, 0x5A, np.uint8).repeat(features.features_dtype().itemsize)
        l = np.full(1, 0x5A, np.uint8).repeat(engine.labels_dtype().itemsize)
        for i in (-1, 6, 1 << 40):
            with pytest.raises(IndexError):
                host_api.dataset_row(h, i, f.ctypes.data, l.ctypes.data)
        assert (f == 0x5A).all() and (l == 0x5A).all()
        host_api.dataset_row(h, 5, None, l.ctypes.data)
        assert l.view(engine.labels_dtype())["did_win"][0] == 1 and (f == 0x5A).all()
    finally:
        host_api.dataset_close(h)
    assert C.sizeof(features.Features) == features.features_dtype().itemsize


# ---- the parser under the sanitizers, as a program of its own ------------------------------------
def test_reader_under_address_and_ub_sanitizers(tmp_path):
    """tests/native/dataset_reader_main.cc over the fixture and every damaged variant, built with
    -fsanitize=address,undefined -fno-sanitize-recover=all (runtimes linked statically) and run as a child process."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the reader's sanitizer program"
    exe = tmp_path / "dataset_reader_main"
    src = os.path.join(dc.ROOT, "tests", "native", "dataset_reader_main.cc")
    # the sanitizer runtimes are linked statically: the program does not care what else the loader brings in, and the
    # child runs in the environment it inherits
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", src, "-o", str(exe), "-lz"], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), dc.FIXTURE], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "0 failures" in r.stdout and "FAIL" not in r.stdout


# ---- the restatement, pinned by hand -------------------------------------------------------------
def test_restatement_hand_cases():
    assert [dr.score_pred_of(a) for a in (0, 399, 400, 799)] == [-399, 0, 0, 399]
    assert [dr.score_pred_of(a) for a in (398, 401)] == [-1, 1]
    v = np.zeros(800, np.float32)
    v[[17, 300, 640]] = 0.25
    assert dr.argmax_ref(v) == 17 and dr.argmax_scan(v) == 17                       # a tie: the first index
    assert dr.argmax_ref(np.full(362, 0.5, np.float32)) == 0
    nan = np.full(362, np.nan, np.float32)
    assert dr.argmax_ref(nan) == 0 and dr.argmax_scan(nan) == 0                     # all NaN: index 0
    nan[200] = -1.0
    nan[201] = -1.0
    assert dr.argmax_ref(nan) == 200 and dr.argmax_scan(nan) == 200                 # NaN never wins
    low = np.full(5, -np.inf, np.float32)
    low[3] = -dr.FLT_MAX
    assert dr.argmax_ref(low) == 0 and dr.argmax_scan(low) == 0                     # nothing above -FLT_MAX: index 0
    rng = np.random.default_rng(5)
    for _ in range(50):
        x = rng.integers(-3, 4, 800).astype(np.float32)
        x[rng.integers(0, 800, 40)] = np.nan
        assert dr.argmax_ref(x) == dr.argmax_scan(x)
    assert dr.ce_loss(0.0) == 16.0 and dr.ce_loss(-0.0) == 16.0
    assert dr.ce_loss(1.0) == 0.0 and dr.ce_loss(np.float32(0.25)) == pytest.approx(np.log(4.0), rel=1e-15)
    assert dr.ce_loss(np.float32(1e-45)) == pytest.approx(103.27892990343184, rel=1e-12)   # the smallest denormal

    mp = np.zeros(362, np.float32)
    mp[[7, 9]] = 0.5
    vp = np.array([0.25, 0.75], np.float32)
    sp = np.zeros(800, np.float32)
    sp[399] = 1
    pol = np.zeros(362, np.float32)
    pol[9] = 1
    t = dr.terms(mp, vp, sp, pol, np.float32(-2.5), 1)
    assert list(t) == [pytest.approx(np.log(2.0)), pytest.approx(-np.log(0.75)), 0.0, 1.0, 2.5, 0.0]
    pol[:] = 0
    pol[7] = 1
    sp[:] = 0
    sp[0] = 1
    t = dr.terms(mp, vp, sp, pol, np.float32(1.5), 0)
    assert list(t[2:]) == [1.0, 0.0, 400.5, -399.0] and t[1] == pytest.approx(np.log(4.0))
    mp[7] = 0
    assert dr.terms(mp, vp, sp, pol, 0.0, 0)[0] == 16.0
    assert list(dr.ulp_distance([1.0, np.nan, 16.0], [1.0 + 2.0 ** -23, np.nan, 16.0])) == [1.0, 0.0, 0.0]


def test_host_scoring_path_equals_the_restatement():
    """p3achygo_amd.dataset.host_terms (the --host-scoring leg of tools/dataset_benchmark.py) is the vectorised twin of
    the restatement: equal on the rows built for the kernels, losses included."""
    from p3achygo_amd import dataset
    mp, vp, sp, lab = dc.synthetic_rows()
    assert np.array_equal(dataset.host_terms(mp, vp, sp, lab), dr.terms_rows(mp, vp, sp, lab))
