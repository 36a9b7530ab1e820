"""No output bit of the engine depends on device memory that the forward pass did not write ("What a forward
pass may read").  p3hip_debug_poison fills every value buffer of an engine (the residual stream, the blocks' and heads'
scratch, q / k / v token rows 0..360, the output rows, result and aux records, the terms and sums of scoring and loss)
with one byte; an engine poisoned in front of every calibration and every run must give, bit for bit, what an engine of
the same file, flags and environment gives that ran the same loads and was never poisoned:
    0xFF  NaN as fp16 and fp32, -1 as int8
    0x7B  about 6.1e4 as fp16, 1.3e36 as fp32, 123 as int8: finite, so it shows what an fmax or a compare hides of a NaN
"Every output": get_raw, the result record's bytes, GetOwnership, GetAux under FLAG_AUX, the INT8 scales after
calibration, and the sums and per-slot terms of score() and loss() where labels and targets are loaded.

A configuration (CONFIGS: one per code path that owns scratch, on the nets that path's own test file uses) runs, on one
engine of batch 24 (low latency: 8): step 1, all slots; step 2, five scattered slots (low latency: three), which
compacts to an odd row count, ragged for every positions-per-workgroup value, with the rows behind it full of the fill.
FLAG_LAUNCH_GRAPH engines run the full batch three times (plain, captured, replayed) before step 2.  Transformers
without symmetries also read q, k and v back after every run: token rows 361..383, which p3hip_create zeroes once and
the hook must leave alone, are still exactly zero.

So that two equally wrong engines cannot agree, step 1 of every poisoned engine is also held against float64 under the
bounds of the plan's own test file, through that file's checker: test_engine_gpu._check, conv_widths_common
.check_outputs with the tables of test_conv_widths_gpu and low_latency_common, fp32_common.check_outputs,
test_transformer_gpu._check / test_transformer_widths_gpu._check on the committed fixtures, and the BOUNDS of the INT8
plan's *_restatement module.  Those INT8 bounds are stated for given positions (the net's golden fixture, or
conv_widths_common.positions()): the slots that hold those positions are checked under them, the other slots by the
bit-for-bit contract alone.  A symmetry-averaged slot is held against the average of the float64 outputs of its copies
(symavg_restatement.expand, rotated back) under the bounds of one copy: the mean of k values that each lie within a
bound lies within it.

Positions: conv_widths_common.positions() (features.random_positions(16, seed=11)) followed by
features.random_positions(16, seed=12); slot s of step 1 holds position s, step 2 loads positions 24.. .  The INT8 plans
with golden-stated bounds put the fixture's positions first; the transformers run their fixtures' positions.

Measured on one MI355X: every configuration is clean under both bytes (DESIGN.md section 19 has the table, and the two
mutations of a local build that turned this file red); the file takes 18 s.

One child process per family (tests/scratch_poison_child.py), each under its own time limit, engines created and closed
one at a time; a failing child fails the tests that need it and nothing is started after it.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_widths_common as cw  # noqa: E402
from conftest import ROOT, load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD = os.path.join(ROOT, "tests", "scratch_poison_child.py")
TIMEOUT = 300   # seconds per child
B, B_LL = 24, 8
STEP2, STEP2_LL = [1, 6, 7, 16, 23], [1, 4, 7]
MASKS = (0x01, 0x35, 0xFF)
PATTERNS = ("ff", "7b")
# engine.FLAG_*
RUN_ALL, GRAPH, INT8, SYM_AVG, INT8_FUSED, INT8_C128, FP32, FP32_TFM = 2, 8, 16, 32, 64, 128, 256, 512
AUX, INT8_ANY, LOW_LAT, LOW_LAT_TFM, SYM_SLOT, INT8_CONV3 = 1024, 2048, 4096, 8192, 16384, 32768


def _runs(batch=B, step2=None, full=1):
    step2 = step2 or (STEP2 if batch == B else STEP2_LL)
    rot = (0, 5, 11)
    runs = [{"slots": list(range(batch)), "pos": [(s + rot[r]) % batch for s in range(batch)]} for r in range(full)]
    return runs + [{"slots": step2, "pos": [B + k for k in range(len(step2))]}]


def _job(key, group, net, check, flags=0, env=None, batch=B, pool="conv", runs=None, **more):
    return dict(key=key, group=group, net=net, check=check, flags=flags, env=env or {}, batch=batch, pool=pool,
                runs=runs or _runs(batch), **more)


def _slot_runs():
    """mixed masks per slot, moved by one between the steps: the packed copies' rows differ from run to run"""
    runs = _runs()
    runs[0]["masks"] = [MASKS[s % 3] for s in runs[0]["slots"]]
    runs[1]["masks"] = [MASKS[(k + 2) % 3] for k in range(len(runs[1]["slots"]))]
    return runs


def _avg_runs():
    runs = _runs()
    for r in runs:
        r["avg"] = 0x35
    return runs


def _cache_runs():
    runs = _runs()
    runs[1]["pos"] = [3, B, 10, B + 1, 17]   # three positions of step 1 (hits) between two new ones
    return runs


FINEST = "finest"   # replaced by the finest stem, dense, heads split of the net's stream (engine.debug_edge_split)
NO_FUSE = {"P3HIP_NO_FUSE": "1", "P3HIP_NO_BFUSE": "1"}
CONFIGS = [
    # fused fp16 (k_block, k_headsx): btl, nbt (d_s), C = 128, broadcast blocks joined into the launch
    _job("fused:b3c256btl1", "fused", "test_b3c256btl1", "engine"),
    _job("fused:b3c256nbt", "fused", "test_b3c256nbt", "engine"),
    _job("fused:b3c128nbt", "fused", "test_b3c128nbt", "engine"),
    _job("fused:b5c256btl2_i2", "fused", "test_b5c256btl2_i2", "engine"),
    _job("fused:b5c128btl1_i2", "fused", "test_b5c128btl1_i2", "engine"),
    _job("fused:b5c256btl2_i2:nofuse", "fused", "test_b5c256btl2_i2", "engine", env=NO_FUSE),
    _job("fused:b5c256btl2_i2:blockw", "fused", "test_b5c256btl2_i2", "blockw", env={"P3HIP_BLOCKW": "1"}, path="Blockw"),
    # layer-wise fp16 (k_lconv, k_heads at C = 384), runtime widths with padded C or C_b (k_lconv_any), fp32
    _job("layer:b3c384btl3", "layer", "test_b3c384btl3", "engine"),
    _job("layer:b3c384nbt", "layer", "test_b3c384nbt", "engine"),
    _job("layer:b3c192classic", "layer", "test_b3c192classic", "engine"),
    _job("any:b3c96nbt", "layer", "test_b3c96nbt", "widths", path="ConvAny"),
    _job("any:b3c320nbt", "layer", "test_b3c320nbt", "widths", path="ConvAny"),
    _job("any:b3c192btl3", "layer", "test_b3c192btl3", "widths", path="ConvAny"),
    _job("fp32:b3c96nbt", "layer", "test_b3c96nbt", "fp32", flags=FP32, path="F32Conv"),
    # INT8: one net per flag, from that flag's own GPU test
    _job("int8:b3c384btl3", "int8", "test_b3c384btl3", "int8", flags=INT8, int8=True, pool="gold:test_b3c384btl3", path="Int8"),
    _job("int8_fused:b3c256btl1", "int8", "test_b3c256btl1", "int8_fused", flags=INT8_FUSED, int8=True,
         pool="gold:test_b3c256btl1", path="Int8Fused256"),
    _job("int8_c128:b3c128btl2", "int8", "test_b3c128btl2", "int8_c128", flags=INT8_C128, int8=True,
         pool="gold:test_b3c128btl2", path="Int8Fused128"),
    _job("int8_any:b3c96nbt", "int8", "test_b3c96nbt", "int8_any", flags=INT8_ANY, int8=True, path="Int8Any"),
    _job("int8_conv3:b3c384btl3", "int8", "test_b3c384btl3", "int8_conv3", flags=INT8_CONV3, int8=True, path="Int8Conv3"),
    _job("int8_conv3:b3c192btl3", "int8", "test_b3c192btl3", "int8_conv3", flags=INT8_CONV3, int8=True, path="Int8Conv3"),
    # transformers: both stream paddings in fp16, fp32, and the low-latency plans with their own and the finest split
    _job("tfm:b2d96h3", "tfm", "test_b2d96h3_tfm", "tfm96", pool="tfm:test_b2d96h3_tfm", tfm=True),
    _job("tfm:b2d64h2", "tfm", "test_b2d64h2_tfm", "tfmw", pool="tfm:test_b2d64h2_tfm", tfm=True),
    _job("fp32_tfm:b2d96h3", "tfm", "test_b2d96h3_tfm", "fp32tfm", flags=FP32_TFM, pool="tfm:test_b2d96h3_tfm", tfm=True,
         path="TfmF32"),
    _job("lowlat_tfm:b2d384h6", "tfm", "test_b2d384h6_tfm", "tfmw", flags=LOW_LAT_TFM, batch=B_LL,
         pool="tfm:test_b2d384h6_tfm", tfm=True, path="TfmSplit"),
    _job("lowlat_tfm:b2d384h6:finest", "tfm", "test_b2d384h6_tfm", "tfmw", flags=LOW_LAT_TFM, batch=B_LL,
         env={"P3HIP_EDGE_SPLIT": FINEST}, pool="tfm:test_b2d384h6_tfm", tfm=True, path="TfmSplit"),
    _job("lowlat:b5c256btl2_i2", "tfm", "test_b5c256btl2_i2", "lowlat", flags=LOW_LAT, batch=B_LL, path="Split"),
    _job("lowlat:b5c256btl2_i2:finest", "tfm", "test_b5c256btl2_i2", "lowlat", flags=LOW_LAT, batch=B_LL,
         env={"P3HIP_EDGE_SPLIT": FINEST}, path="Split"),
    # symmetries: the copies' rows in d_feats and d_cout, whose packing changes between the steps
    _job("sym_avg:b3c256btl1", "sym", "test_b3c256btl1", "engine", flags=SYM_AVG, runs=_avg_runs()),
    _job("sym_avg:b3c384nbt", "sym", "test_b3c384nbt", "engine", flags=SYM_AVG, runs=_avg_runs()),
    _job("sym_slot:b3c256btl1", "sym", "test_b3c256btl1", "engine", flags=SYM_SLOT, runs=_slot_runs()),
    _job("sym_slot:b3c384nbt", "sym", "test_b3c384nbt", "engine", flags=SYM_SLOT, runs=_slot_runs()),
]
# on top of one fused and one layer-wise net
for _net, _tag in (("test_b3c256btl1", "b3c256btl1"), ("test_b3c384btl3", "b3c384btl3")):
    CONFIGS += [
        _job("aux:" + _tag, "ontop", _net, "engine", flags=AUX, labels=True),
        _job("run_all:" + _tag, "ontop", _net, "engine", flags=RUN_ALL),
        _job("graph:" + _tag, "ontop", _net, "engine", flags=GRAPH, runs=_runs(full=3)),
        _job("cache:" + _tag, "ontop", _net, "engine", cache=6, runs=_cache_runs()),
    ]
KEYS = [c["key"] for c in CONFIGS]
BY_KEY = {c["key"]: c for c in CONFIGS}
GROUPS = ["fused", "layer", "int8", "tfm", "sym", "ontop"]


def _is_tfm(net):
    return net.endswith("_tfm")


def _weights(net):
    from p3achygo_amd import netspec
    if net == "test_b2d96h3_tfm":
        from tfm_restatement import fixture_weights
        return fixture_weights(net)
    if _is_tfm(net):
        from tfm_restatement_dh import fixture_weights
        return fixture_weights(net)
    cfg = netspec.get_config(net)
    return cfg, netspec.generate_weights(cfg, randomize=True)


def _c_pad(cfg):
    if cfg.block_type == "transformer":
        return 128 if cfg.channels <= 128 else 256 if cfg.channels <= 256 else 384
    return cw.padded(cfg.channels)


_POOLS = {}


def _pool(pool):
    """(positions [32], index of each in its reference: the fixture's row, or itself)"""
    from p3achygo_amd import features
    if pool not in _POOLS:
        conv = np.concatenate([cw.positions(), features.random_positions(16, seed=12)])
        kind, _, net = pool.partition(":")
        if kind == "conv":
            _POOLS[pool] = (conv, np.arange(32))
        elif kind == "gold":   # the conv fixture's few positions first
            _, gpos = load_golden(net)
            _POOLS[pool] = (np.concatenate([gpos, conv])[:32], np.arange(32))
        else:                  # a transformer's fixture, as many times over as it takes
            _, gpos = load_golden(net)
            idx = np.arange(32) % len(gpos)
            _POOLS[pool] = (gpos[idx], idx)
    return _POOLS[pool]


def _labels_and_targets():
    from p3achygo_amd import engine
    rng = np.random.default_rng(2024)

    def dist(n):
        p = rng.random((32, n)) ** 4
        return (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
    lab = np.zeros(32, engine.labels_dtype())
    lab["policy"], lab["score_margin"], lab["did_win"] = dist(362), rng.integers(-60, 61, 32), rng.integers(0, 2, 32)
    tg = np.zeros(32, engine.targets_dtype())
    tg["policy"], tg["policy_aux_dist"], tg["mcts_value_dist"] = dist(362), dist(362), dist(51)
    tg["own"] = rng.integers(-1, 2, (32, 361))
    tg["score_margin"] = rng.integers(-60, 61, 32)
    for k in ("q6", "q16", "q50"):
        tg[k], tg[k + "_score"] = rng.uniform(-1, 1, 32), rng.uniform(-40, 40, 32)
    tg["policy_aux"], tg["has_pi_aux_dist"], tg["has_mcts_value_dist"] = rng.integers(0, 362, 32), 1, 1
    return lab, tg


@pytest.fixture(scope="module")
def children(built, tmp_path_factory):
    """group -> the outputs of that group's child, run once on first use; a failure is kept and raised again"""
    import int8_restatement as ir
    from p3achygo_amd import engine, netspec
    tmp = tmp_path_factory.mktemp("scratch_poison")
    done, paths = {}, {}

    def path_of(net):
        if net not in paths:
            cfg, W = _weights(net)
            paths[net] = str(tmp / (net + ".p3w"))
            netspec.save_p3w(paths[net], cfg, W)
        return paths[net]

    def run(group):
        if group not in done and any(isinstance(v, BaseException) for v in done.values()):
            pytest.fail("an earlier child failed: no further GPU process is started")
        if group not in done:
            jobs = []
            for c in (c for c in CONFIGS if c["group"] == group):
                cfg, _ = _weights(c["net"])
                job = {k: c[k] for k in ("key", "flags", "batch", "pool", "runs")}
                job.update(path=path_of(c["net"]), int8=c.get("int8", False), cache=c.get("cache"), labels=c.get("labels", False))
                job["env"] = {k: ("%d,%d,%d" % engine.debug_edge_split(1, _c_pad(cfg)) if v == FINEST else v)
                              for k, v in c["env"].items()}
                if c.get("tfm"):
                    job["tfm"] = [cfg.bottleneck_channels, cfg.channels // cfg.bottleneck_channels]
                if c.get("path"):   # the configuration runs the plan it is here for
                    os.environ.update(job["env"])
                    try:
                        assert engine.debug_plan(job["path"], c["flags"])[0] == c["path"], c["key"]
                    finally:
                        for k in job["env"]:
                            del os.environ[k]
                jobs.append(job)
            lab, tg = _labels_and_targets()
            spec = {"labels": np.frombuffer(lab.tobytes(), np.uint8), "targets": np.frombuffer(tg.tobytes(), np.uint8)}
            for pool in {j["pool"] for j in jobs}:
                spec["pool:" + pool] = np.frombuffer(_pool(pool)[0].tobytes(), np.uint8)
            for b, cal in enumerate(ir.calibration_batches()):
                spec["calib:%d" % b] = np.frombuffer(cal.tobytes(), np.uint8)
            inp, outp, jobp = tmp / f"in_{group}.npz", tmp / f"out_{group}.npz", tmp / f"jobs_{group}.json"
            np.savez(inp, **spec)
            jobp.write_text(json.dumps(jobs))
            env = {k: v for k, v in os.environ.items() if not k.startswith("P3HIP_") or k == "P3HIP_LIB"}
            try:
                r = subprocess.run([sys.executable, CHILD, str(inp), str(outp), str(jobp)], env=env, capture_output=True,
                                   text=True, timeout=TIMEOUT)
                assert r.returncode == 0, f"child {group}: exit {r.returncode}\n{r.stdout[-600:]}\n{r.stderr[-3000:]}"
                with np.load(outp) as z:
                    done[group] = {k: z[k] for k in z.files}
            except BaseException as exc:   # noqa: BLE001 - kept for the other tests of this child, nothing runs again
                done[group] = exc
        if isinstance(done[group], BaseException):
            raise done[group]
        return done[group]
    return run


def _differing(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return "shapes %s and %s" % (a.shape, b.shape)
    if a.tobytes() == b.tobytes():
        return None
    av, bv = a.reshape(len(a), -1), b.reshape(len(b), -1)
    bad = np.argwhere((av.view(np.uint8) != bv.view(np.uint8)).reshape(len(a), -1))
    rows = sorted({int(r) for r in bad[:, 0]})
    first = bad[0]
    return "%d bytes differ in rows %s, the first at row %d byte %d" % (len(bad), rows[:12], first[0], first[1])


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("key", KEYS)
def test_poisoned_engine_gives_the_clean_engines_bits(children, key, pattern):
    c = BY_KEY[key]
    out = children(c["group"])
    what = ["raw", "own", "rec", "hit", "state"] + (["aux"] if c["flags"] & AUX else []) + \
        (["score", "loss"] if c.get("labels") else []) + (["zero"] if c.get("tfm") else [])
    if c.get("int8"):
        clean, got = out[f"{key}:clean:scales"], out[f"{key}:{pattern}:scales"]
        assert len(clean) > 0 and (clean > 0).all() and np.isfinite(clean).all()
        assert _differing(got[None], clean[None]) is None, ("scales", got, clean)
    for r, run in enumerate(c["runs"]):
        n = len(run["slots"])
        raw = out[f"{key}:clean:{r}:raw"]
        # the clean engine's rows are worth comparing: finite, not constant, one per loaded slot
        assert raw.shape == (n, 1889) and np.isfinite(raw).all() and (np.abs(raw).max(axis=1) > 0).all()
        assert len({row.tobytes() for row in raw}) == len({p for p in _pool(c["pool"])[1][run["pos"]]})
        for w in what:
            d = _differing(out[f"{key}:{pattern}:{r}:{w}"], out[f"{key}:clean:{r}:{w}"])
            assert d is None, f"{key} poisoned with 0x{pattern}, run {r} ({n} slots), {w}: {d}"
        assert np.array_equal(out[f"{key}:{pattern}:{r}:own"], raw[:, 1526:1887])
        if c.get("tfm"):   # q, k, v token rows 361..383: zeroed once, and still zero
            assert out[f"{key}:{pattern}:{r}:zero"].all() and out[f"{key}:clean:{r}:zero"].all()
        if c.get("labels"):
            assert out[f"{key}:clean:{r}:score"][6] == n and out[f"{key}:clean:{r}:loss"][19] == n
            assert np.isfinite(out[f"{key}:clean:{r}:score"]).all() and np.isfinite(out[f"{key}:clean:{r}:loss"]).all()
    if c["flags"] & GRAPH:   # plain, captured, replayed, then the kernel-by-kernel run of five
        assert [int(out[f"{key}:{pattern}:{r}:state"][0]) for r in range(4)] == [0, 1, 1, 1]
    if c.get("cache"):   # the hits of step 2 are the records step 1 stored, not bytes of d_out
        hit = out[f"{key}:{pattern}:1:hit"]
        assert hit.tolist() == [True, False, True, False, True] and not out[f"{key}:{pattern}:0:hit"].any()
        for k in (0, 2, 4):
            p = c["runs"][1]["pos"][k]
            for w in ("raw", "rec"):
                assert out[f"{key}:{pattern}:1:{w}"][k].tobytes() == out[f"{key}:{pattern}:0:{w}"][p].tobytes(), (key, k, w)


# ---- step 1 against float64 -----------------------------------------------------------------------------------------

_REFS = {}


def _conv_reference(net, pos):
    cfg, W = _weights(net)
    return cw.outputs(cfg, W, pos, fp16=False)


def _sym_reference(net, pos, masks):
    """row i: the average over the symmetries of masks[i] of the float64 outputs of position i's copies, rotated back"""
    import symavg_restatement as sr
    from p3achygo_amd import engine
    fwd = engine.symmetry_maps()[0]
    copies = np.concatenate([sr.expand(pos[i:i + 1], m, fwd) for i, m in enumerate(masks)])
    o = _conv_reference(net, copies)
    board = {"raw": (0, 362, 1526), "move_probs": (0,), "opt_move_probs": (0,), "value_probs": (), "score_probs": ()}
    ref = {k: np.zeros((len(pos),) + o[k].shape[1:]) for k in o}
    at = 0
    for i, m in enumerate(masks):
        syms = sr.syms_of(m)
        for j, s in enumerate(syms):
            mp = fwd[s].astype(np.int64)
            for k, starts in board.items():
                row = np.array(o[k][at + j], np.float64)
                for b in starts:
                    row[b:b + 361] = o[k][at + j][b + mp]
                ref[k][i] += row / len(syms)
        at += len(syms)
    return ref


def _reference(c):
    """{raw, the four distributions} in float64, one row per slot of step 1"""
    run = c["runs"][0]
    sym = tuple(run.get("masks") or ([run["avg"]] * c["batch"] if run.get("avg") else ()))
    key = (c["net"], c["pool"], c["batch"], sym, c["check"] == "fp32tfm")
    if key not in _REFS:
        pos, idx = _pool(c["pool"])
        pos, idx = pos[run["pos"]], idx[run["pos"]]
        if c["check"] == "fp32tfm":
            import tfm_fp32_common as tc
            import tfm_restatement_dh as dh
            cfg, W = tc.weights(c["net"])
            _, planes, scalars = tc.inputs(c["net"])
            o = dh.forward(cfg, W, planes[idx], scalars[idx])
            _REFS[key] = {k: np.asarray(o[k], np.float64) for k in ("raw",) + cw.PROB_KEYS}
        elif _is_tfm(c["net"]):
            g, _ = load_golden(c["net"])
            _REFS[key] = {k: np.asarray(g[k], np.float64)[idx] for k in ("raw",) + cw.PROB_KEYS}
        elif c["pool"].startswith("gold:"):   # the fixture's rows as committed, the restatement for the others
            g, gpos = load_golden(c["net"])
            ref = _conv_reference(c["net"], pos)
            for k in ref:
                ref[k][:len(gpos)] = np.asarray(g[k], np.float64)
            _REFS[key] = ref
        elif sym:
            _REFS[key] = _sym_reference(c["net"], pos, sym)
        else:
            _REFS[key] = _conv_reference(c["net"], pos)
    return _REFS[key]


def _int8_bounds(check, net):
    import int8_any_restatement
    import int8_block_c128
    import int8_block_restatement
    import int8_conv3_restatement
    import int8_restatement
    mod = {"int8": int8_restatement, "int8_fused": int8_block_restatement, "int8_c128": int8_block_c128,
           "int8_any": int8_any_restatement, "int8_conv3": int8_conv3_restatement}[check]
    # the positions the bounds are stated for: the fixture's (at the front of a "gold:" pool), or cw.positions()
    n = len(load_golden(net)[1]) if check in ("int8", "int8_fused", "int8_c128") else cw.NPOS
    return mod.BOUNDS[net], n


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("key", KEYS)
def test_step_1_of_the_poisoned_engine_against_float64(children, key, pattern):
    import fp32_common as fc
    import int8_restatement as ir
    import low_latency_common as ll
    import test_conv_widths_gpu as tcw
    import test_engine_gpu as teg
    import test_transformer_gpu as ttg
    import test_transformer_widths_gpu as ttw
    from p3achygo_amd import features
    c = BY_KEY[key]
    out = children(c["group"])
    raw, own = out[f"{key}:{pattern}:0:raw"], out[f"{key}:{pattern}:0:own"]
    recs = [features.Result.from_buffer_copy(r.tobytes()) for r in out[f"{key}:{pattern}:0:rec"]]
    ref, net, check = _reference(c), c["net"], c["check"]
    n = c["batch"]
    assert raw.shape == (n, 1889) == ref["raw"].shape and len(recs) == n   # no slot is left out of the comparison
    if check.startswith("int8"):
        bounds, m = _int8_bounds(check, net)
        got = {"raw": raw[:m].astype(np.float64),
               "move_probs": np.stack([np.ctypeslib.as_array(r.move_probs) for r in recs[:m]]).astype(np.float64),
               "value_probs": np.stack([np.ctypeslib.as_array(r.value_probs) for r in recs[:m]]).astype(np.float64)}
        err = ir.errors(got, {k: ref[k][:m] for k in got})
        print(f"{key} 0x{pattern}: {err} (bounds {bounds}, {m} positions)")
        assert np.isfinite(raw).all()
        for k, bound in bounds.items():
            assert err[k] <= bound, (key, err)
        return
    worst = float(np.abs(raw - ref["raw"]).max())
    print(f"{key} 0x{pattern}: largest raw-output error {worst:.3e} over {n} slots")
    if check == "blockw":   # test_engine_gpu.test_hand_scheduled_block_kernel_matches_the_fixtures_and_the_hip_kernels
        assert not np.isnan(raw).any() and teg._logits_close(raw[:, :1887], ref["raw"][:, :1887]), key
        return
    tol = {"widths": tcw.TOL, "lowlat": ll.tolerances()}.get(check, {}).get(net)
    idx = _pool(c["pool"])[1][c["runs"][0]["pos"]]
    g = load_golden(net)[0] if check in ("tfm96", "tfmw") else None
    for i in range(n):
        if check == "engine":
            teg._check(raw[i], recs[i], ref["raw"][i], {k: ref[k][i] for k in teg.PROB_KEYS})
            assert np.abs(own[i] - ref["raw"][i][1526:1887]).max() <= teg.LOGIT_TOL
        elif check in ("widths", "lowlat"):
            cw.check_outputs(net, tol, raw[i], recs[i], ref, i)
        elif check in ("fp32", "fp32tfm"):
            import tfm_fp32_common as tc
            rt, pt = (fc.RAW_TOL, fc.PROB_TOL) if check == "fp32" else (tc.RAW_TOL, tc.PROB_TOL)
            fc.check_outputs(net, raw[i], recs[i], own[i], ref, i, rt, pt)
        elif check == "tfm96":
            ttg._check(net, raw[i], recs[i], g, int(idx[i]))
        elif check == "tfmw":
            ttw._check(net, raw[i], recs[i], g, int(idx[i]))
        else:
            raise AssertionError(check)
