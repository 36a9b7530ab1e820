"""The policy / value head kernels at trained-net magnitudes, every instantiation (kernels.hip k_headsx<C,32,V>,
k_heads<32,V>; the fp32 plans' k_heads), teacher-forced: p3hip_get_raw of an engine that ran to the end against heads()
in float64 on that engine's own x (p3hip_debug_x), and the result record (GetBatch) against the engine's own logits.

The weights are tests/heads_common.py sharp_heads: gamma on both sides of the softplus' branch at 20 and of the clamp at
10, a q6_err logit below -89 (where __expf(-s) overflows) and above +20, outcome logits 30 and more apart, saturated
ownership, every head mish on both asymptotes, peaked policies and score distributions.  Every job is a one-block net at
batch 41 (a ragged tail for the four-position workgroups of k_heads and the two-position ones of k_headsx);
heads_common.JOBS lists them: the six k_headsx instantiations, the four of k_heads, k_heads behind P3HIP_NO_HFUSE, the
any-width kernels (C = 64, 512 and the padded 96), both fp32 plans, the three transformer streams, and a hot trunk
(trunk_emulation.hot_weights: x in the hundreds) under each kernel.  The regimes are asserted on the float64 reference
before an engine output is looked at (heads_common.assert_coverage).

The measure is, per raw segment and position, max |got - want| / max(1, max |want| over the segment); the bounds
(heads_common.BOUNDS, PROB_BOUNDS) come from the float32 twin on the CPU (tests/test_heads_cpu.py), none from an engine.
The fp32 engines must also be no further from the float64 net (the whole net from the positions, nothing rounded) than
the fp16 engine on the same net, segment by segment.

Each environment (default, P3HIP_NO_HFUSE=1) runs in one child process under its own time limit, engines created and
closed one at a time; a failing child fails the tests that need it, nothing retries.

Measured on one MI355X (57 tests, 20 s wall for the whole file, the calibration on the CPU included): worst error per
segment over the jobs of a family, and the twin's on the same x (the engines' own, so not the CPU file's figures):
                  pi       opt      outcome  score    ownership  q6_err   gamma
    twin          3.07e-6  5.09e-6  2.22e-6  2.36e-5  1.02e-5    2.33e-5  2.20e-5
    k_headsx      4.21e-6  6.95e-6  8.88e-7  1.83e-5  3.42e-6    5.02e-5  2.23e-5
    k_heads       7.11e-6  1.73e-5  2.20e-6  2.21e-5  6.37e-6    2.86e-5  2.61e-5
    fp32          4.68e-6  1.33e-5  2.45e-6  2.10e-5  6.77e-6    4.04e-5  2.92e-5
    bound         8.8e-5   1.3e-4   4.4e-5   1.1e-3   3.6e-4     1.6e-3   9.5e-4
Every family stays at least 7 times inside every bound.  The largest ratio of an engine's worst to the twin's on the same
x is 10.1 (c384v48nbt opt: 1.73e-5 against 1.71e-6; the same net's pi is 3.8); over a family it is 3.4 (k_heads opt).
Against the float64 net the fp32 engines are at 8.8e-8 .. 3.8e-5 where the fp16 engines are at 4.7e-5 .. 2.3e-2.  The
record's probabilities are within 3.0e-7 of the float64 softmax of the engine's logits (bounds 1.4e-6 .. 4.9e-6), finite
and summing to one on every slot; q6_err is exactly 0 wherever its logit is below -89.  No kernel fault was found.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import heads_common as hc  # noqa: E402
from conftest import ROOT  # noqa: E402

pytestmark = pytest.mark.gpu

TIMEOUTS = {"": 420, "P3HIP_NO_HFUSE": 150}   # seconds per child
RECORD_KEYS = ("move_logits", "move_probs", "value_probs", "score_probs", "opt_move_probs")

_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from p3achygo_amd import engine, features
d = np.load(sys.argv[1], allow_pickle=True)
pos = np.frombuffer(d["pos"].tobytes(), dtype=features.features_dtype()).copy()
n = len(pos)
out = {}
for key in d["keys"]:
    eng = engine.HipEngine(d[key + ":path"].item(), n, flags=int(d[key + ":flags"]))
    eng.load_all(pos)
    eng.RunInference()
    out[key + ":x"] = eng.debug_x(n, int(d[key + ":Cs"]))[:, :int(d[key + ":C"])]
    out[key + ":raw"] = np.stack([eng.get_raw(s) for s in range(n)])
    recs = [features.result_to_dict(eng.GetBatch(s)) for s in range(n)]
    for f in %r:
        out[key + ":" + f] = np.stack([r[f] for r in recs])
    out[key + ":err2_outcome"] = np.array([r["err2_outcome"] for r in recs], np.float32)
    eng.close()
np.savez(sys.argv[2], **out)
"""


@pytest.fixture(scope="module")
def children(built, tmp_path_factory):
    """env -> the outputs of that environment's child, run once on first use; a failure is kept and raised again"""
    from p3achygo_amd import engine, netspec
    tmp = tmp_path_factory.mktemp("heads")
    pos = hc.positions()
    done = {}

    def run(env_name):
        if env_name not in done and any(isinstance(v, BaseException) for v in done.values()):
            pytest.fail("an earlier child failed: no further GPU process is started")
        if env_name not in done:
            jobs = [j for j in hc.JOBS if j.env == env_name]
            spec = {"keys": np.array([j.name for j in jobs]), "pos": np.frombuffer(pos.tobytes(), np.uint8)}
            for j in jobs:
                cfg, _, W = hc.weights(j.net, pos)
                path = str(tmp / (j.net.replace(":", "_") + ".p3w"))
                if not os.path.exists(path):
                    netspec.save_p3w(path, cfg, W)
                flags = 0 if not j.fp32 else (engine.FLAG_FP32_TFM if hc.is_tfm(cfg) else engine.FLAG_FP32)
                spec.update({j.name + ":path": np.array(path), j.name + ":flags": np.array(flags),
                             j.name + ":C": np.array(cfg.channels), j.name + ":Cs": np.array(hc.stream_width(cfg))})
            inp, outp = tmp / f"in_{env_name}.npz", tmp / f"out_{env_name}.npz"
            np.savez(inp, **spec)
            env = {k: v for k, v in os.environ.items()
                   if k not in ("P3HIP_NO_HFUSE", "P3HIP_NO_FUSE", "P3HIP_NO_BFUSE", "P3HIP_DEBUG_STOP_BLOCK", "P3HIP_CONV_ANY")}
            if env_name:
                env[env_name] = "1"
            try:
                r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, RECORD_KEYS), str(inp), str(outp)], env=env,
                                   capture_output=True, text=True, timeout=TIMEOUTS[env_name])
                assert r.returncode == 0, f"child {env_name or 'default'}: exit {r.returncode}\n{r.stderr[-3000:]}"
                done[env_name] = dict(np.load(outp))
            except BaseException as exc:   # noqa: BLE001 - kept for the other tests of this child, nothing runs again
                done[env_name] = exc
        if isinstance(done[env_name], BaseException):
            raise done[env_name]
        return done[env_name]
    return run


_EVAL = {}


def _evaluate(children, job):
    """(x, want, got, per-position errors, the twin's errors on the same x) of a job, once; the regimes of the float64
    reference are asserted before the engine's output is read"""
    if job.name not in _EVAL:
        out = children(job.env)
        cfg, _, W = hc.weights(job.net)
        x = np.asarray(out[job.name + ":x"], np.float64).reshape(hc.BATCH, cfg.channels, 19, 19)
        want = hc.reference(cfg, W, x, job.fp32)
        hc.assert_coverage(hc.coverage(want, hc.probs64(want), hc.stages(x, hc.head_weights(W, job.fp32))), job.name)
        low = hc.stages(x, hc.head_weights(W, job.fp32))["go"][:, 5] < -89    # __expf(-s) is inf: 4 / (1 + inf)
        got = np.asarray(out[job.name + ":raw"], np.float64)
        assert low.any() and np.all(got[low, 1887] == 0), (job.name, "q6_err below -89", got[low, 1887])
        _EVAL[job.name] = (x, want, got, hc.segment_errors(got, want),
                           hc.segment_errors(hc.twin_raw(cfg, W, x, job.fp32), want))
    return _EVAL[job.name]


@pytest.mark.parametrize("job", hc.JOBS, ids=lambda j: j.name)
def test_raw_outputs_on_the_engines_own_x(children, job):
    x, want, got, errs, twin = _evaluate(children, job)
    if job.net.endswith(":hot"):
        assert np.abs(x).max() > 100
    print(f"{job.name} [{job.family}]: " + " ".join(f"{k} {errs[k].max():.2e} (twin {twin[k].max():.2e})" for k in hc.SEG_NAMES))
    assert np.isfinite(got).all(), (job.name, np.argwhere(~np.isfinite(got))[:8])
    hc.check_raw(job.name, got, want)
    if job.fp32:
        # no further from the float64 net than the fp16 engine on the same net.  Both against the whole net in float64
        # from the positions (unrounded weights, no fp16 anywhere): teacher-forced, the two errors are float32 summation
        # noise of the same size (the CPU twin measures 5.9e-6 for fp32 and 3.7e-6 for fp16 on pi of c256v64nbt), and
        # which of them is larger says nothing.
        cfg, _, W = hc.weights(job.net)
        exact = hc.reference(cfg, W, hc.trunk_x(cfg, W, hc.positions(), fp16=False), fp32=True)
        got16 = _evaluate(children, next(j for j in hc.JOBS if j.net == job.net and not j.fp32 and not j.env))[2]
        e32, e16 = hc.worst(hc.segment_errors(got, exact)), hc.worst(hc.segment_errors(got16, exact))
        print(f"{job.name} against the float64 net: " + " ".join(f"{k} {e32[k]:.2e} (fp16 {e16[k]:.2e})" for k in hc.SEG_NAMES))
        for k in hc.SEG_NAMES:
            assert e32[k] <= e16[k], (job.name, k, f"fp32 {e32[k]:.3g} fp16 {e16[k]:.3g}")


@pytest.mark.parametrize("job", hc.JOBS, ids=lambda j: j.name)
def test_result_record_against_the_engines_own_logits(children, job):
    out = children(job.env)
    raw = out[job.name + ":raw"]
    worst = dict.fromkeys(hc.PROB_KEYS, 0.0)
    for s in range(hc.BATCH):
        rec = {f: out[f"{job.name}:{f}"][s] for f in RECORD_KEYS + ("err2_outcome",)}
        for k, v in hc.record_check(raw[s], rec, f"{job.name} slot {s}").items():
            worst[k] = max(worst[k], v)
    print(f"{job.name} record: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_report(children):
    """information: the worst error per segment of the twin and of each kernel family, and the largest ratio of an
    engine's worst to the twin's on the same x (jobs whose child failed are left out)"""
    fam, ratio = {}, (0.0, "")
    for job in hc.JOBS:
        try:
            _, _, _, errs, twin = _evaluate(children, job)
        except BaseException:   # noqa: BLE001 - reported by the job's own test
            continue
        for f, e in ((job.family, errs), ("twin", twin)):
            row = fam.setdefault(f, dict.fromkeys(hc.SEG_NAMES, 0.0))
            for k in hc.SEG_NAMES:
                row[k] = max(row[k], float(e[k].max()))
        for k in hc.SEG_NAMES:
            r = float(errs[k].max() / twin[k].max()) if twin[k].max() > 0 else 0.0
            if r > ratio[0]:
                ratio = (r, f"{job.name} {k}: {errs[k].max():.3g} against {twin[k].max():.3g}")
    print("family      " + " ".join(f"{k:>10}" for k in hc.SEG_NAMES))
    for f in ("twin", "k_headsx", "k_heads", "fp32"):
        if f in fam:
            print(f"{f:<12}" + " ".join(f"{fam[f][k]:10.2e}" for k in hc.SEG_NAMES))
    print("bound       " + " ".join(f"{hc.BOUNDS[k]:10.2e}" for k in hc.SEG_NAMES))
    print(f"largest engine / twin ratio: {ratio[0]:.2f} ({ratio[1]})")
