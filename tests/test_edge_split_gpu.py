"""The split stem, broadcast dense and heads of the two low-latency plans (csrc/edge_split.hip) on
the HIP engine, through the C ABI.  Everything here is byte equality, no tolerance anywhere: an engine with the chooser's
split, or with any (s, d, h) of the sets forced through P3HIP_EDGE_SPLIT, against the reference leg, an engine created
under P3HIP_EDGE_SPLIT=0 (the unsplit launches), and for the transformers against a default-plan engine (no flag).  What
is compared per slot: the raw floats (p3hip_get_raw), the p3hip_result record and the ownership; and the residual stream x
after the stem and after the first broadcast block (P3HIP_DEBUG_STOP_BLOCK).

The environment is read at p3hip_create, so the engines run in a child process (tests/edge_split_child.py), one per test.

test_b2d96h3_tfm has a 128-channel stream (one stem pass: nothing of the stem to split) and k_headsx for its heads, which
stays whole: a forced split changes no launch there, and the test says that the bytes stay the default plan's.
test_b2d192h6_tfm (stream 256, k_headsx) is the transformer whose stem alone splits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conftest import ROOT  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD = os.path.join(ROOT, "tests", "edge_split_child.py")
CONV_NETS = ["test_b3c64btl2", "test_b3c128btl2", "test_b3c256nbt", "test_b4c512btl3_i2"]
COMPOSE_NET = "test_b3c256nbt"
N_CU = 256   # MI355X


def _config(name):
    from p3achygo_amd import netspec
    return netspec.get_config(name)


def _c_pad(cfg):
    if cfg.block_type == "transformer":
        return 128 if cfg.channels <= 128 else 256 if cfg.channels <= 256 else 384
    return (cfg.channels + 63) // 64 * 64


def _sets(c_pad):
    """every (s, d, h) of the documented sets (csrc/edge_split.h) for a stream of c_pad channels"""
    passes = c_pad // (128 if c_pad % 128 == 0 else 64)
    return ["%d,%d,%d" % (s, d, h) for s in sorted({1, passes}) for d in (1, 3, 12) for h in (1, 4, 8)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> .p3w of netspec.generate_weights(cfg, randomize=True), written on demand"""
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("edge_split")
    cache = {}

    def get(name):
        if name not in cache:
            cfg = _config(name)
            cache[name] = os.path.join(d, name + ".p3w")
            netspec.save_p3w(cache[name], cfg, netspec.generate_weights(cfg, randomize=True))
        return cache[name]
    return get


def _run(tmp_path, jobs):
    outp, jobp = tmp_path / "out.npz", tmp_path / "jobs.json"
    jobp.write_text(json.dumps(jobs))
    env = {k: v for k, v in os.environ.items() if k not in ("P3HIP_EDGE_SPLIT", "P3HIP_DEBUG_STOP_BLOCK", "P3HIP_SPLIT",
                                                           "P3HIP_TFM_SPLIT")}
    r = subprocess.run([sys.executable, CHILD, str(outp), str(jobp)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    with np.load(outp) as z:   # (read now: a test may run a second child into the same directory)
        return {k: z[k] for k in z.files}


def _same(got, key, want_key, what):
    a, b = got[key], got[want_key]
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), (what, key, np.argwhere(a != b)[:5].tolist())


def _alive(rows):
    """a result worth comparing: the raw floats of every row are finite and not all zero"""
    raw = rows[:, :1889].view(np.float32)
    assert np.isfinite(raw).all() and (np.abs(raw).max(axis=1) > 0).all()


def _crossover(c_pad):
    from p3achygo_amd import engine
    return next(n for n in range(1, 4096) if engine.debug_edge_split(n, c_pad, N_CU) == (1, 1, 1))


@pytest.mark.parametrize("name", CONV_NETS)
def test_conv_outputs_are_the_unsplit_launches_bytes(built, files, tmp_path, name):
    """batches 1, 3, 8 and the first batch at which the chooser splits nothing: the chooser's own split and every forced
    (s, d, h) of the sets give the raw floats, the result record and the ownership of every slot of the reference leg"""
    from p3achygo_amd import engine
    c_pad = _c_pad(_config(name))
    past = _crossover(c_pad)
    assert engine.debug_edge_split(8, c_pad, N_CU) != (1, 1, 1) and past > 8
    F = engine.FLAG_LOW_LATENCY
    legs = ["0", None] + _sets(c_pad)
    jobs = [dict(key="%d:%s" % (b, leg), path=files(name), batch=b, flags=F, env={} if leg is None else {"P3HIP_EDGE_SPLIT": leg})
            for b in (1, 3, 8, past) for leg in legs]
    got = _run(tmp_path, jobs)
    for b in (1, 3, 8, past):
        _alive(got["%d:0:0" % b])
        for leg in legs[1:]:
            _same(got, "%d:%s:0" % (b, leg), "%d:0:0" % b, name)
    # the same position gives the same bytes at every batch size (slot s holds position s mod 16)
    assert got["3:None:0"][:1].tobytes() == got["1:None:0"].tobytes()
    assert got["8:None:0"][:3].tobytes() == got["3:None:0"].tobytes()


@pytest.mark.parametrize("name", CONV_NETS)
def test_conv_stream_after_the_stem_and_the_first_broadcast_block(built, files, tmp_path, name):
    """x after the stem (P3HIP_DEBUG_STOP_BLOCK=0) and after the first broadcast block, at batch 3: the chooser's split
    and every forced one against the reference leg"""
    from p3achygo_amd import engine
    cfg = _config(name)
    c_pad = _c_pad(cfg)
    first_bc = next(i for i in range(cfg.blocks) if cfg.block_kind(i) == "broadcast")
    F = engine.FLAG_LOW_LATENCY
    legs = ["0", None] + _sets(c_pad)
    jobs = []
    for stop in (0, first_bc + 1):
        for leg in legs:
            env = {"P3HIP_DEBUG_STOP_BLOCK": str(stop)}
            if leg is not None:
                env["P3HIP_EDGE_SPLIT"] = leg
            jobs.append(dict(key="%d:%s" % (stop, leg), path=files(name), batch=3, flags=F, env=env, x=c_pad))
    got = _run(tmp_path, jobs)
    for stop in (0, first_bc + 1):
        want = got["%d:0:x" % stop]
        assert np.isfinite(want).all() and np.abs(want[:, :cfg.channels]).max() > 0
        for leg in legs[1:]:
            _same(got, "%d:%s:x" % (stop, leg), "%d:0:x" % stop, (name, stop))
    assert got["0:0:x"].tobytes() != got["%d:0:x" % (first_bc + 1)].tobytes()


@pytest.mark.parametrize("name,stem_splits,heads_split", [("test_b2d384h6_tfm", True, True), ("test_b2d192h6_tfm", True, False),
                                                          ("test_b2d96h3_tfm", False, False)])
def test_transformer_outputs_and_stem_are_the_default_plans_bytes(built, files, tmp_path, name, stem_splits, heads_split):
    """P3HIP_FLAG_LOW_LATENCY_TFM with the chooser's split and with forced ones against a DEFAULT-PLAN engine (no flag),
    the guarantee the plan already gives: raw outputs at batches 1, 3 and 8, and x after the stem.  stream 384, V = 80:
    k_heads, stem and heads split; stream 256: k_headsx, the stem alone; stream 128: one stem pass and k_headsx, nothing
    splits and a forced heads split is ignored"""
    from p3achygo_amd import engine
    cfg = _config(name)
    c_pad = _c_pad(cfg)
    passes = c_pad // 128
    assert (passes > 1) == stem_splits
    F = engine.FLAG_LOW_LATENCY_TFM
    assert engine.debug_plan(files(name), F)[0] == "TfmSplit" and engine.debug_plan(files(name), 0)[0] == "Tfm"
    legs = ["0", None] + ["%d,1,%d" % (s, h) for s in sorted({1, passes}) for h in (1, 4, 8)]
    jobs = []
    for b in (1, 3, 8):
        jobs.append(dict(key="%d:default" % b, path=files(name), batch=b, flags=0))
        jobs += [dict(key="%d:%s" % (b, leg), path=files(name), batch=b, flags=F, env={} if leg is None else {"P3HIP_EDGE_SPLIT": leg})
                 for leg in legs]
    jobs.append(dict(key="x:default", path=files(name), batch=3, flags=0, env={"P3HIP_DEBUG_STOP_BLOCK": "0"}, x=c_pad))
    for leg in legs:
        env = {"P3HIP_DEBUG_STOP_BLOCK": "0"}
        if leg is not None:
            env["P3HIP_EDGE_SPLIT"] = leg
        jobs.append(dict(key="x:%s" % leg, path=files(name), batch=3, flags=F, env=env, x=c_pad))
    got = _run(tmp_path, jobs)
    for b in (1, 3, 8):
        _alive(got["%d:default:0" % b])
        for leg in legs:
            _same(got, "%d:%s:0" % (b, leg), "%d:default:0" % b, name)
    assert np.abs(got["x:default:x"]).max() > 0
    for leg in legs:
        _same(got, "x:%s:x" % leg, "x:default:x", name)
    if not heads_split:   # k_headsx: the heads' parts are not looked at
        assert engine.debug_plan(files(name), F)[0] == "TfmSplit"


def _compose(tmp_path, files, extra, **kw):
    """COMPOSE_NET at batch 8 with `extra` flags: the chooser's split and the finest forced one against the reference leg"""
    from p3achygo_amd import engine
    F = engine.FLAG_LOW_LATENCY | extra
    jobs = [dict(key=k, path=files(COMPOSE_NET), batch=8, flags=F, env=env, **kw)
            for k, env in (("ref", {"P3HIP_EDGE_SPLIT": "0"}), ("own", {}), ("fine", {"P3HIP_EDGE_SPLIT": "2,12,8"}))]
    return _run(tmp_path, jobs)


def test_launch_graph_replays_bit_for_bit(built, files, tmp_path):
    """eager, capture, then three replays (graph_state 1): every round equals the reference leg's"""
    from p3achygo_amd import engine
    got = _compose(tmp_path, files, engine.FLAG_LAUNCH_GRAPH, loads=[list(range(8))] * 5)
    for k in ("ref", "own", "fine"):
        assert got[k + ":g"].tolist() == [0, 1, 1, 1, 1], (k, got[k + ":g"])
    _alive(got["ref:0"])
    for r in range(5):
        for k in ("own", "fine"):
            _same(got, "%s:%d" % (k, r), "ref:0", r)
    # and an engine without the graph gives those bytes too
    plain = _compose(tmp_path, files, 0)
    assert plain["own:0"].tobytes() == got["ref:0"].tobytes()


def test_compaction_of_5_of_8_slots(built, files, tmp_path):
    part = [0, 2, 3, 5, 7]
    got = _compose(tmp_path, files, 0, loads=[list(range(8)), part])
    _alive(got["ref:1"])
    assert got["ref:1"].tobytes() == got["ref:0"][part].tobytes()
    for k in ("own", "fine"):
        _same(got, k + ":0", "ref:0", k)
        _same(got, k + ":1", "ref:1", k)


def test_aux_record_and_every_other_output(built, files, tmp_path):
    from p3achygo_amd import engine
    got = _compose(tmp_path, files, engine.FLAG_AUX, aux=True)
    plain = _compose(tmp_path, files, 0)
    _alive(got["ref:0"])
    assert np.isfinite(got["ref:aux"]).all() and np.abs(got["ref:aux"]).max() > 0
    assert got["ref:0"].tobytes() == plain["ref:0"].tobytes()
    for k in ("own", "fine"):
        _same(got, k + ":0", "ref:0", k)
        _same(got, k + ":aux", "ref:aux", k)


def test_symmetry_averaging_with_mask_0x35(built, files, tmp_path):
    """four copies per slot: the passes run 32 rows, the pooled-values buffer is sized for 8 x the batch"""
    from p3achygo_amd import engine
    got = _compose(tmp_path, files, engine.FLAG_SYMMETRY_AVG, sym=0x35)
    _alive(got["ref:0"])
    for k in ("own", "fine"):
        _same(got, k + ":0", "ref:0", k)


@pytest.mark.parametrize("name,batch,split", [("test_b3c64btl2", 40, "1,12,8"), ("test_b4c512btl3_i2", 80, "4,12,8")])
def test_more_items_than_one_round(built, files, tmp_path, name, batch, split):
    """the finest split forced at a batch whose items pass the CUs, so that the item loops wrap (C = 64: 480 items of the
    dense; C = 512: 320 of the stem, 3840 of the dense): every slot is bit-identical to its position in a batch-8 run"""
    from p3achygo_amd import engine
    c_pad = _c_pad(_config(name))
    s, d, h = (int(v) for v in split.split(","))
    assert batch * max(s, d * ((c_pad + 127) // 128)) > N_CU
    F = engine.FLAG_LOW_LATENCY
    jobs = [dict(key="small", path=files(name), batch=8, flags=F, env={"P3HIP_EDGE_SPLIT": "0"}, mod=8),
            dict(key="big", path=files(name), batch=batch, flags=F, env={"P3HIP_EDGE_SPLIT": split}, mod=8)]
    got = _run(tmp_path, jobs)
    _alive(got["small:0"])
    want = got["small:0"][np.arange(batch) % 8]
    assert got["big:0"].tobytes() == want.tobytes(), np.argwhere(got["big:0"] != want)[:5].tolist()
