"""The fifteen aux outputs on the device (P3HIP_FLAG_AUX, csrc/heads_aux.hip k_heads_aux, p3hip_get_aux), teacher-forced:
the 41 records of an engine that ran to the end against the float64 restatement (tests/aux_common.py aux_stages) on that
engine's own x (p3hip_debug_x), per segment under the bounds the CPU test derives from the float32 twin; then what the
flag must leave alone and what the entry point must do: the other outputs bit for bit, compaction, the captured graph,
no residue between runs, the refusals.

One job per head-conv family (aux_common.JOBS): the fused heads' extra conv launch at C = 128 and 256, k_heads at V = 80,
the classic trunk, the any-width kernels with padded C and C_b, both transformer stream paddings, both fp32 plans, and an
INT8 plan after a calibration run.  The weights are heads_common.sharp_heads' with aux_common.sharp_aux on top: tanh
inputs to +-12, sigmoid inputs below -89 and above +20, both signs in front of abs, bin logits near +100 with a bin above
0.9, peaked aux and soft policies; the regimes are asserted on the float64 reference before an engine output is read.

Two child processes, each under its own time limit, engines created and closed one at a time; a failing child fails the
tests that need it and nothing is started after it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import aux_common as ac  # noqa: E402
import heads_common as hc  # noqa: E402
from conftest import ROOT  # noqa: E402

pytestmark = pytest.mark.gpu

TIMEOUTS = {"jobs": 300, "behaviour": 240}   # seconds per child
FUSED_NET, UNFUSED_NET = "c256v48btl", "c384v80nbt"
SCATTER = [0, 3, 4, 9, 13, 17, 22, 23, 29, 31, 38, 40, 47, 52, 57, 62, 63]   # 17 of 64 slots

_PRELUDE = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np
from p3achygo_amd import engine, features
d = np.load(sys.argv[1], allow_pickle=True)
pos = np.frombuffer(d["pos"].tobytes(), dtype=features.features_dtype()).copy()
n = len(pos)
out = {}
def aux_of(eng, slots):
    recs = [eng.GetAux(s) for s in slots]
    assert all(r is not None for r in recs), [s for s, r in zip(slots, recs) if r is None]
    return np.stack(recs)
def result_bytes(eng, slots):
    return np.stack([np.frombuffer(bytes(eng.GetBatch(s)), np.uint8) for s in slots])
"""

_JOBS = _PRELUDE + r"""
for key in d["keys"]:
    flags = int(d[key + ":flags"])
    eng = engine.HipEngine(d[key + ":path"].item(), n, flags=flags)
    if flags & engine.FLAG_INT8_C128:
        eng.load_all(pos)
        eng.int8_calibrate()
    eng.load_all(pos)
    eng.RunInference()
    out[key + ":x"] = eng.debug_x(n, int(d[key + ":Cs"]))[:, :int(d[key + ":C"])]
    out[key + ":aux"] = aux_of(eng, range(n))
    out[key + ":raw"] = np.stack([eng.get_raw(s) for s in range(n)])
    eng.close()
np.savez(sys.argv[2], **out)
"""

_BEHAVIOUR = _PRELUDE + r"""
AUX = engine.FLAG_AUX
def run(path, batch, flags, slots, positions):
    eng = engine.HipEngine(path, batch, flags=flags)
    for s, p in zip(slots, positions):
        eng.LoadBatch(s, pos[p:p + 1])
    eng.RunInference()
    return eng

# flag on against flag off: get_raw and the result record of every slot
for net in ("fused", "unfused"):
    path = d[net + ":path"].item()
    for flags in (0, AUX):
        eng = run(path, n, flags, range(n), range(n))
        out[f"{net}:{flags}:raw"] = np.stack([eng.get_raw(s) for s in range(n)])
        if flags:
            out[f"{net}:aux"] = aux_of(eng, range(n))
        out[f"{net}:{flags}:rec"] = result_bytes(eng, range(n))
        if flags:   # all_outputs of one slot, beside get_raw and GetAux of the same run
            eng.LoadBatch(0, pos[0:1])
            eng.RunInference()
            out[f"{net}:all0:raw"], out[f"{net}:all0:aux"] = eng.get_raw(0), eng.GetAux(0)
            names = eng.all_outputs(0)
            out[f"{net}:names"] = np.array(list(names))
            out[f"{net}:all0"] = np.concatenate([np.ravel(v) for v in names.values()]).astype(np.float32)
        eng.close()

path = d["fused:path"].item()
scatter = [int(s) for s in d["scatter"]]
# compaction: 17 scattered slots of a 64-slot engine against the same positions alone in a batch-1 engine
eng = run(path, 64, AUX, scatter, range(len(scatter)))
out["compact:aux"] = aux_of(eng, scatter)
out["compact:unloaded"] = np.array([eng._L.p3hip_get_aux(eng._h, s, np.zeros(837, np.float32).ctypes.data)
                                    for s in range(64) if s not in scatter])
keep = np.full(837, 7.5, np.float32)
rc = eng._L.p3hip_get_aux(eng._h, 1, keep.ctypes.data)
out["compact:untouched"] = np.array([rc == 2 and bool((keep == 7.5).all())])
out["compact:bad_slot"] = np.array([eng._L.p3hip_get_aux(eng._h, s, keep.ctypes.data) for s in (-1, 64)])
out["compact:get_slot_after"] = result_bytes(eng, scatter)
out["compact:aux_after_fetch"] = aux_of(eng, scatter)
try:
    eng.EnableCache(8)
    out["cache:error"] = np.array("")
except engine.EngineError as exc:
    out["cache:error"] = np.array(str(exc))
eng.close()
one = engine.HipEngine(path, 1, flags=AUX)
alone = []
for p in range(len(scatter)):
    one.LoadBatch(0, pos[p:p + 1])
    one.RunInference()
    alone.append(one.GetAux(0))
    one.GetBatch(0)
out["alone:aux"] = np.stack(alone)
one.close()
plain = engine.HipEngine(path, 1, flags=0)
plain.LoadBatch(0, pos[0:1])
plain.RunInference()
out["plain:rc"] = np.array([plain._L.p3hip_get_aux(plain._h, 0, keep.ctypes.data)])
plain.close()
eng = run(path, 64, AUX | engine.FLAG_RUN_ALL_SLOTS, scatter, range(len(scatter)))
out["runall:aux"] = aux_of(eng, scatter)
eng.close()

# the captured graph: a full batch of 8, run twice with different positions
for flags in (AUX, AUX | engine.FLAG_LAUNCH_GRAPH):
    eng = run(path, 8, flags, range(8), range(8))
    first = aux_of(eng, range(8))
    result_bytes(eng, range(8))
    for s in range(8):
        eng.LoadBatch(s, pos[8 + s:9 + s])
    eng.RunInference()
    out[f"graph:{flags & engine.FLAG_LAUNCH_GRAPH}:state"] = np.array([eng.graph_state()])
    out[f"graph:{flags & engine.FLAG_LAUNCH_GRAPH}:aux"] = np.stack([first, aux_of(eng, range(8))])
    eng.close()

# residue: a second run over fewer, other positions against a fresh engine that ran only those
eng = run(path, n, AUX, range(n), range(n))
result_bytes(eng, range(n))
second = list(range(n - 1, n - 21, -1))
for s, p in enumerate(second):
    eng.LoadBatch(s, pos[p:p + 1])
eng.RunInference()
out["residue:second"] = aux_of(eng, range(20))
out["residue:stale"] = np.array([eng.GetAux(s) is None for s in range(20, n)])
eng.close()
eng = run(path, n, AUX, range(20), second)
out["residue:fresh"] = aux_of(eng, range(20))
eng.close()

# a pass stopped in front of the heads computes no record
os.environ["P3HIP_DEBUG_STOP_BLOCK"] = "1"
eng = run(path, 4, AUX, range(4), range(4))
del os.environ["P3HIP_DEBUG_STOP_BLOCK"]
out["stopped:rc"] = np.array([eng._L.p3hip_get_aux(eng._h, s, keep.ctypes.data) for s in range(4)])
eng.close()
np.savez(sys.argv[2], **out)
"""


@pytest.fixture(scope="module")
def children(built, tmp_path_factory):
    """name -> the outputs of that child, run once on first use; a failure is kept and raised again"""
    from p3achygo_amd import engine, netspec
    tmp = tmp_path_factory.mktemp("aux")
    pos = hc.positions()
    done = {}

    def path_of(net):
        cfg, W = ac.weights(net, pos)
        path = str(tmp / (net + ".p3w"))
        if not os.path.exists(path):
            netspec.save_p3w(path, cfg, W)
        return cfg, path

    def run(name):
        if name not in done and any(isinstance(v, BaseException) for v in done.values()):
            pytest.fail("an earlier child failed: no further GPU process is started")
        if name not in done:
            spec = {"pos": np.frombuffer(pos.tobytes(), np.uint8)}
            if name == "jobs":
                spec["keys"] = np.array([j.name for j in ac.JOBS])
                for j in ac.JOBS:
                    cfg, path = path_of(j.net)
                    flags = engine.FLAG_AUX | {"fp16": 0, "int8": engine.FLAG_INT8_C128,
                                               "fp32": engine.FLAG_FP32_TFM if hc.is_tfm(cfg) else engine.FLAG_FP32}[j.plan]
                    spec.update({j.name + ":path": np.array(path), j.name + ":flags": np.array(flags),
                                 j.name + ":C": np.array(cfg.channels), j.name + ":Cs": np.array(hc.stream_width(cfg))})
            else:
                spec.update({"fused:path": np.array(path_of(FUSED_NET)[1]), "unfused:path": np.array(path_of(UNFUSED_NET)[1]),
                             "scatter": np.array(SCATTER)})
            inp, outp = tmp / f"in_{name}.npz", tmp / f"out_{name}.npz"
            np.savez(inp, **spec)
            env = {k: v for k, v in os.environ.items()
                   if k not in ("P3HIP_NO_HFUSE", "P3HIP_NO_FUSE", "P3HIP_NO_BFUSE", "P3HIP_DEBUG_STOP_BLOCK", "P3HIP_CONV_ANY")}
            try:
                r = subprocess.run([sys.executable, "-c", (_JOBS if name == "jobs" else _BEHAVIOUR) % ROOT, str(inp), str(outp)],
                                   env=env, capture_output=True, text=True, timeout=TIMEOUTS[name])
                assert r.returncode == 0, f"child {name}: exit {r.returncode}\n{r.stderr[-3000:]}"
                done[name] = dict(np.load(outp))
            except BaseException as exc:   # noqa: BLE001 - kept for the other tests of this child, nothing runs again
                done[name] = exc
        if isinstance(done[name], BaseException):
            raise done[name]
        return done[name]
    return run


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("job", ac.JOBS, ids=lambda j: j.name)
def test_records_on_the_engines_own_x(children, job):
    """Measured on one MI355X, worst error per segment over the jobs of a family: DESIGN.md section 13."""
    out = children("jobs")
    cfg, W = ac.weights(job.net)
    x = np.asarray(out[job.name + ":x"], np.float64).reshape(hc.BATCH, cfg.channels, 19, 19)
    st = ac.aux_stages(x, hc.head_weights(W, job.fp32))
    want = st["rec"]
    ac.assert_coverage(ac.coverage(want, st), job.name)
    got = np.asarray(out[job.name + ":aux"], np.float64)
    assert got.shape == (hc.BATCH, ac.AUX_LEN) == want.shape   # no position is left out of the comparison
    twin = ac.worst(ac.segment_errors(ac.twin_rec(W, x, job.fp32), want))
    errs = ac.worst(ac.segment_errors(got, want))
    print(f"{job.name} [{job.family}]: " + " ".join(f"{k} {errs[k]:.2e} (twin {twin[k]:.2e})" for k in ac.SEG_NAMES) +
          f" softmax {ac.prob_errors(got).max():.2e}")
    assert np.isfinite(got).all(), (job.name, np.argwhere(~np.isfinite(got))[:8])
    ac.check_rec(job.name, got, want)
    low = st["go"][:, 6:8] < -89   # __expf(-s) is inf there: 4 / (1 + inf)
    assert low.any() and np.all(got[:, 727:729][low] == 0), (job.name, got[:, 727:729][low])
    # the outputs the engine had before are still those of heads_common on the same x
    hc.check_raw(job.name, out[job.name + ":raw"], hc.reference(cfg, W, x, job.fp32))


@pytest.mark.parametrize("net", ["fused", "unfused"])
def test_flag_leaves_the_other_outputs_bit_identical(children, net):
    from p3achygo_amd import engine
    out = children("behaviour")
    on, off = engine.FLAG_AUX, 0
    assert out[f"{net}:{on}:raw"].shape == (hc.BATCH, 1889)
    assert _same_bits(out[f"{net}:{on}:raw"], out[f"{net}:{off}:raw"])
    assert out[f"{net}:{on}:rec"].shape[0] == hc.BATCH and _same_bits(out[f"{net}:{on}:rec"], out[f"{net}:{off}:rec"])
    # all_outputs: the 25 names in order, slot 0's values those of get_raw and GetAux
    assert list(out[f"{net}:names"]) == ac.output_names()
    parts = dict(zip(ac.output_names(), np.split(out[f"{net}:all0"], np.cumsum(
        [362, 362, 2, 2, 361, 800, 800, 1, 362, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 362, 362, 51, 51])[:-1])))
    raw, rec = out[f"{net}:all0:raw"], out[f"{net}:all0:aux"]
    assert _same_bits(parts["00:pi_logits"], raw[:362]) and _same_bits(parts["22:pi_logits_optimistic"], raw[362:724])
    assert _same_bits(parts["12:q6_err"], raw[1887:1888]) and _same_bits(parts["04:own"], raw[1526:1887])
    assert _same_bits(parts["08:pi_logits_aux"], rec[:362]) and _same_bits(parts["24:mcts_dist_probs"], rec[786:])
    assert abs(parts["01:pi"].sum() - 1) < 1e-4 and abs(parts["06:score_probs"].sum() - 1) < 1e-4


def test_compaction(children):
    out = children("behaviour")
    assert out["compact:aux"].shape == (len(SCATTER), ac.AUX_LEN)
    assert _same_bits(out["compact:aux"], out["alone:aux"])
    assert _same_bits(out["runall:aux"], out["alone:aux"])
    assert len(out["compact:unloaded"]) == 64 - len(SCATTER) and (out["compact:unloaded"] == 2).all()
    assert out["compact:untouched"].all()
    assert (out["compact:bad_slot"] == 1).all() and (out["plain:rc"] == 1).all()
    assert out["compact:get_slot_after"].shape[0] == len(SCATTER)          # p3hip_get_slot still succeeds after it
    assert _same_bits(out["compact:aux_after_fetch"], out["compact:aux"])   # and the record stays until the next run
    # the records differ between positions: the comparison is not of constants
    assert len({r.tobytes() for r in out["compact:aux"]}) == len(SCATTER)


def test_cache_is_refused_on_an_aux_engine(children):
    msg = str(children("behaviour")["cache:error"])
    assert "not available on a P3HIP_FLAG_AUX engine" in msg and "no room for the aux record" in msg, msg


def test_launch_graph(children):
    from p3achygo_amd import engine
    out = children("behaviour")
    g = engine.FLAG_LAUNCH_GRAPH
    assert out[f"graph:{g}:state"][0] == 1 and out["graph:0:state"][0] == 0
    assert out[f"graph:{g}:aux"].shape == (2, 8, ac.AUX_LEN)
    assert _same_bits(out[f"graph:{g}:aux"], out["graph:0:aux"])
    # the replayed run's records are the second positions', not what the first run left
    assert not _same_bits(out[f"graph:{g}:aux"][0], out[f"graph:{g}:aux"][1])


def test_second_run_shows_no_residue(children):
    out = children("behaviour")
    assert out["residue:second"].shape == (20, ac.AUX_LEN)
    assert _same_bits(out["residue:second"], out["residue:fresh"])
    assert out["residue:stale"].all()   # slots the second run did not evaluate answer 2


def test_stopped_pass_has_no_record(children):
    assert (children("behaviour")["stopped:rc"] == 2).all()
