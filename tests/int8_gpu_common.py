"""What the INT8 GPU tests share (tests/test_int8_gpu.py, test_int8_block_gpu.py, test_int8_c128_gpu.py,
test_int8_any_gpu.py, test_int8_conv3_gpu.py): engines of one INT8 flag, calibrated or with the scales of one that was,
their outputs as arrays like the goldens, the fixture weights and oracle outputs, the positions of a teacher-forced job
and the child process of one.

Every engine is calibrated on int8_restatement.calibration_batches() (seeded random positions, apart from every
evaluated set); the other restatements re-export that very function.  What differed between the files' copies is an
explicit argument here: the flag, whether `raw` comes back as float64 (the goldens' type) or as the engine's float32 (for
comparisons bit for bit), and whether a calibrated engine takes the flag on top of `flags` or `flags` alone.

TEST INFRASTRUCTURE ONLY."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT, load_golden  # noqa: E402
import int8_restatement as ir  # noqa: E402

_SCALES = {}   # (flag, path) -> calibrated scales: two flags calibrate the same file differently


class Engines:
    """The engines of one INT8 flag (`flag`: the name of the constant in p3achygo_amd.engine, read at first use so that
    importing a test file does not load the library).  raw_f64: `raw` of fetch() and run() as float64."""

    def __init__(self, flag, raw_f64):
        self._flag, self.raw_f64 = flag, raw_f64

    def flag(self):
        from p3achygo_amd import engine
        return getattr(engine, self._flag)

    def calibrated(self, path, batch, flags=0, own=True):
        """own: the engine's flags are this flag | flags; not own: `flags` alone (another plan, calibrated the same way)"""
        from p3achygo_amd import engine
        eng = engine.HipEngine(path, batch, flags=(self.flag() if own else 0) | flags)
        for cal in ir.calibration_batches():
            assert len(cal) <= batch
            eng.load_all(cal)
            eng.int8_calibrate()
            for i in range(len(cal)):
                eng.GetBatch(i)
        return eng

    def scales(self, path):
        """The calibrated scales of the net at `path` (one calibration per flag, file and session)."""
        key = (self.flag(), path)
        if key not in _SCALES:
            eng = self.calibrated(path, 16)
            _SCALES[key] = eng.int8_scales()
            eng.close()
        return _SCALES[key]

    def with_scales(self, path, batch, flags=0):
        from p3achygo_amd import engine
        eng = engine.HipEngine(path, batch, flags=self.flag() | flags)
        eng.set_int8_scales(self.scales(path))
        return eng

    def fetch(self, eng, slots):
        raw = np.stack([eng.get_raw(s) for s in slots])
        res = [eng.GetBatch(s) for s in slots]
        return {"raw": raw.astype(np.float64) if self.raw_f64 else raw,
                "move_probs": np.stack([np.ctypeslib.as_array(r.move_probs) for r in res]).astype(np.float64),
                "value_probs": np.stack([np.ctypeslib.as_array(r.value_probs) for r in res]).astype(np.float64)}

    def run(self, eng, pos, slots=None):
        """outputs of `pos` loaded at `slots` (default 0..n-1) as arrays like the goldens"""
        slots = list(range(len(pos))) if slots is None else slots
        for k, s in enumerate(slots):
            eng.LoadBatch(s, pos[k:k + 1])
        eng.RunInference()
        return self.fetch(eng, slots)


def weights(name, peak=0.0):
    from p3achygo_amd import netspec
    cfg = netspec.CONFIGS[name]
    W = netspec.generate_weights(cfg, randomize=True)
    return cfg, (netspec.peak_policy(W, peak) if peak else W)


def oracle_outputs(path, pos):
    from oracle import oracle
    net = oracle.OracleNet(path)
    res, raw = net.forward_features(pos)
    return net, {"raw": np.asarray(raw, np.float64),
                 "move_probs": np.stack([np.ctypeslib.as_array(r.move_probs) for r in res]).astype(np.float64),
                 "value_probs": np.stack([np.ctypeslib.as_array(r.value_probs) for r in res]).astype(np.float64)}


def job_batch(name, batch):
    """Positions of a job: the fixture's first positions scattered among seeded fill; the compared slots."""
    from p3achygo_amd import features
    _, gpos = load_golden(name)
    special = gpos[:min(4, batch)]
    pos = features.random_positions(batch, seed=43, n_games=16, max_moves=300, komis=(7.5, -7.5, 0.5))
    at = [int(s) for s in np.linspace(0, batch - 1, len(special)).round()] if batch > 1 else [0]
    pos[at] = special[:len(at)]
    slots = sorted(set(at) | set(range(5, batch, 97)) | {batch - 1})
    return pos, np.asarray(slots)


def child(script, args, failed, timeout, env_extra=None):
    """One child process under its own time limit, nothing retried; once one failed no further one is started.
    failed: the calling file's list of failures so far."""
    if failed:
        pytest.fail("an earlier child failed: no further GPU process is started (%s)" % failed[0])
    env = {k: v for k, v in os.environ.items()
           if k not in ("P3HIP_NO_HFUSE", "P3HIP_NO_FUSE", "P3HIP_NO_BFUSE", "P3HIP_DEBUG_STOP_BLOCK", "P3HIP_CONV_ANY")}
    env.update(env_extra or {})
    try:
        r = subprocess.run([sys.executable, "-c", script % ROOT] + [str(a) for a in args], env=env, capture_output=True,
                           text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        failed.append("time limit")
        raise
    if r.returncode != 0:
        failed.append("exit %d" % r.returncode)
    assert r.returncode == 0, r.stderr[-3000:]
