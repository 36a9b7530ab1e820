"""Results that do not depend on where a position lands in a batch, at the batch sizes where the launch geometry changes.

The launchers switch forms on the batch size and the device's CU count n (csrc/kernels.hip, forward.cpp block_args):
k_block's grid cap (n workgroups for C = 256, 2n for C = 128), k_lconv's pair_split (grid > n), the start-up stagger
(from 3n positions for C = 256, 6n for C = 128), the C = 128 pair turns (from 4n), grid_for's cap at n, and the ragged
tails of k_heads (4 positions per workgroup) and k_headsx (2).  The sweep runs every trunk family on both sides of each
switch and asks for every slot's outputs to equal, bit for bit, those of the same position in a 61-position reference
run — the forward pass of a row does not depend on the other rows of its batch.  61 is prime and slot s of a run over
N positions holds position (7 s + N) mod 61, so no period of the batch lines up with a workgroup or a token tile.
The reference runs themselves are checked against the float64 oracle (the transformer against its golden fixture)
with the bounds of tests/test_engine_gpu.py / tests/test_transformer_gpu.py.

The row-limit tests fill an engine past the row where an activation row's element offset passes 2^31: the fp16 conv
epilogues address x as (uniform base) + (32-bit lane offset), and a lane offset that counted whole positions wrapped
there (residual loads from, and stores into, the first rows of the same buffer).  They need ~20 GB of device memory
each; an engine that cannot get it is skipped with the allocator's message."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden
from test_engine_gpu import PROB_KEYS, _check
import test_transformer_gpu as tfm_gpu

pytestmark = pytest.mark.gpu

NPOS = 61                                  # distinct positions of a reference run: prime
HIP_ATTR_MULTIPROCESSOR_COUNT = 63         # hipDeviceAttributeMultiprocessorCount (hip/hip_runtime_api.h)
RECORD_FIELDS = ("move_logits", "move_probs", "value_probs", "score_probs", "opt_move_probs")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _slot_positions(n):
    return (7 * np.arange(n) + n) % NPOS


def _first_wrapped_row(C):
    """the first activation row (C fp16 channels x 361 points) whose elements reach past 2^31"""
    return (2 ** 31 - 1) // (C * 361)


def _row_limit_rows(C):
    return _first_wrapped_row(C) + 65


def _out(eng, s):
    """one slot's outputs as raw bits: the raw head outputs and every value of the result record"""
    raw = eng.get_raw(s)
    r = eng.GetBatch(s)
    rec = [np.ctypeslib.as_array(getattr(r, f)) for f in RECORD_FIELDS] + [np.float32([r.err2_outcome])]
    return np.concatenate([raw] + rec).astype(np.float32).view(np.uint32)


def _run(eng, pos, idx):
    """loads pos[idx[s]] at slot s and runs"""
    for s, p in enumerate(idx):
        eng.LoadBatch(s, pos[p:p + 1])
    eng.RunInference()


def _mismatches(eng, ref, idx):
    return [s for s, p in enumerate(idx) if not np.array_equal(_out(eng, s), ref[p])]


def _reference(eng, pos):
    _run(eng, pos, range(NPOS))
    return np.stack([_out(eng, s) for s in range(NPOS)])


@pytest.fixture(scope="module")
def n_cu(built):
    """CU count of device 0 as the engine's launchers see it (hipDeviceProp_t::multiProcessorCount), read from the HIP
    runtime libp3hip.so has loaded: a partitioned device shows fewer CUs than 256."""
    from p3achygo_amd import engine
    engine.lib()
    with open("/proc/self/maps") as f:
        hip = sorted({ln.split()[-1] for ln in f if "libamdhip64.so" in ln})
    assert hip, "libp3hip.so did not load the HIP runtime"
    rt = ctypes.CDLL(hip[0], mode=os.RTLD_NOLOAD | os.RTLD_GLOBAL)
    v = ctypes.c_int(0)
    assert rt.hipDeviceGetAttribute(ctypes.byref(v), HIP_ATTR_MULTIPROCESSOR_COUNT, 0) == 0
    assert v.value > 0
    return v.value


@pytest.fixture(scope="module")
def positions(built):
    """61 positions: openings through late game, komi 7.5 / -7.5 / 0.5, a third of them from pass-heavy games"""
    from p3achygo_amd import features
    a = features.random_positions(41, seed=61, n_games=41, max_moves=330, komis=(7.5, -7.5, 0.5))
    b = features.random_positions(20, seed=67, n_games=20, min_moves=120, max_moves=360, pass_prob=0.3,
                                  komis=(7.5, -7.5, 0.5))
    return np.concatenate([a, b])


def _sizes(n):
    return sorted({1, 2, 3, 5, 63, n - 1, n + 1, 2 * n - 1, 2 * n + 1, 3 * n - 1, 3 * n, 4 * n - 1, 4 * n,
                   6 * n - 1, 6 * n, 8 * n + 3})


def _oracle_checked_reference(path, pos):
    from oracle import oracle
    from p3achygo_amd import engine
    eng = engine.HipEngine(path, NPOS)
    ref = _reference(eng, pos)
    res, raw = oracle.OracleNet(path).forward_features(pos, nthreads=8)
    for i in range(NPOS):
        want = {k: np.ctypeslib.as_array(getattr(res[i], k)) for k in PROB_KEYS}
        _check(eng.get_raw(i), eng.GetBatch(i), raw[i], want)
    eng.close()
    return ref


def _sweep(path, pos, ref, sizes, tight, flags=0, setup=None):
    """every size through slot compaction on one engine of the largest size, and `tight` on an engine of exactly that
    batch; every slot bit for bit equal to the reference of its position"""
    from p3achygo_amd import engine
    bad = {}
    for batch, runs in ((max(sizes), sizes), (tight, [tight])):
        eng = engine.HipEngine(path, batch, flags=flags)
        if setup:
            setup(eng)
        for n in runs:
            idx = _slot_positions(n)
            _run(eng, pos, idx)
            m = _mismatches(eng, ref, idx)
            if m:
                bad[(batch, n)] = (len(m), m[:8])
        eng.close()
    assert not bad, "(engine batch, positions run): (slots differing from the reference, first of them): %s" % bad


@pytest.mark.parametrize("name", ["test_b5c128btl1_i2", "test_b3c128nbt", "test_b5c256btl2_i2", "test_b3c256nbt",
                                  "test_b3c384btl3", "test_b3c192classic"])
def test_conv_trunks_are_independent_of_the_batch_geometry(built, weight_files, n_cu, positions, name):
    path = weight_files(name)
    ref = _oracle_checked_reference(path, positions)
    _sweep(path, positions, ref, _sizes(n_cu), 2 * n_cu + 1)


def test_transformer_is_independent_of_the_batch_geometry(built, n_cu, tmp_path):
    """odd sizes move the phase of k_tfm_*'s 64-token tiles against the positions"""
    from p3achygo_amd import engine, netspec
    from tfm_restatement import fixture_weights
    name = "test_b2d96h3_tfm"
    g, gpos = load_golden(name)
    cfg, W = fixture_weights(name)
    path = str(tmp_path / (name + ".p3w"))
    netspec.save_p3w(path, cfg, W)
    pos = gpos[:NPOS]
    eng = engine.HipEngine(path, NPOS)
    ref = _reference(eng, pos)
    for i in range(NPOS):
        tfm_gpu._check(name, eng.get_raw(i), eng.GetBatch(i), g, i)
    eng.close()
    _sweep(path, pos, ref, _sizes(n_cu), 2 * n_cu + 1)


def test_int8_trunk_is_independent_of_the_batch_geometry(built, weight_files, n_cu, positions):
    """FLAG_INT8 with one fixed set of scales (p3hip_int8_set_scales) on every engine"""
    from p3achygo_amd import engine
    path = weight_files("test_b3c384btl3")
    cal = engine.HipEngine(path, NPOS, flags=engine.FLAG_INT8)
    cal.load_all(positions)
    cal.int8_calibrate()
    for i in range(NPOS):
        cal.GetBatch(i)
    scales = cal.int8_scales()
    cal.set_int8_scales(scales)
    ref = _reference(cal, positions)
    cal.close()
    _sweep(path, positions, ref, _sizes(n_cu), 2 * n_cu + 1, engine.FLAG_INT8, lambda e: e.set_int8_scales(scales))


@pytest.mark.parametrize("name", ["test_b3c256btl1", "test_b3c384nbt"])
def test_symmetry_averaged_evaluation_is_independent_of_the_batch_geometry(built, weight_files, n_cu, positions, name):
    """FLAG_SYMMETRY_AVG: 8 rows per slot, so batches around n/8, 3n/8 and 6n/8 put the row counts across the switches"""
    from p3achygo_amd import engine
    path = weight_files(name)
    eng = engine.HipEngine(path, NPOS, flags=engine.FLAG_SYMMETRY_AVG)
    ref = _reference(eng, positions)
    eng.close()
    e = n_cu // 8
    sizes = sorted({1, 5, e, e + 1, 3 * e, 3 * e + 1, 6 * e - 1, 6 * e + 1})
    _sweep(path, positions, ref, sizes, 3 * e + 1 if (3 * e + 1) % 2 else 3 * e + 2,
           engine.FLAG_SYMMETRY_AVG)


def _big_engine(path, batch, flags=0):
    """an engine of `batch` slots, or a skip if the device cannot hold its buffers"""
    from p3achygo_amd import engine
    try:
        return engine.HipEngine(path, batch, flags=flags)
    except engine.EngineError as err:
        if "out of memory" in str(err).lower():
            pytest.skip("batch %d: %s" % (batch, err))
        raise


def _row_report(bad, first_wrapped, what="rows", first=64):
    """bad rows (or slots) in three groups: the first ones (where wrapped stores land), those at or past the row whose
    element offset passes 2^31, and the rest"""
    low = [r for r in bad if r < first]
    high = [r for r in bad if r >= first_wrapped]
    other = [r for r in bad if first <= r < first_wrapped]
    return ("%s 0-%d differing: %d %s; %s from %d on (element offset past 2^31) differing: %d %s; other %s differing: "
            "%d %s" % (what, first - 1, len(low), low[:8], what, first_wrapped, len(high), high[:8], what, len(other),
                       other[:8]))


@pytest.mark.parametrize("name,C", [("test_b3c128btl2", 128), ("test_b3c192classic", 192), ("test_b3c256btl1", 256),
                                    ("test_b3c384btl3", 384)])
def test_rows_past_the_32_bit_element_offset(built, weight_files, positions, name, C):
    from p3achygo_amd import engine
    path = weight_files(name)
    eng = engine.HipEngine(path, NPOS)
    ref = _reference(eng, positions)
    eng.close()
    rows = _row_limit_rows(C)
    eng = _big_engine(path, rows)
    idx = _slot_positions(rows)
    _run(eng, positions, idx)
    bad = _mismatches(eng, ref, idx)
    eng.close()
    assert not bad, _row_report(bad, _first_wrapped_row(C))


def test_symmetry_averaged_c384_batch_past_the_32_bit_element_offset(built, weight_files, positions):
    """the configuration an evaluation net meets: C = 384, all eight symmetries, 8 x batch rows past the limit"""
    from p3achygo_amd import engine
    path = weight_files("test_b3c384nbt")
    eng = engine.HipEngine(path, NPOS, flags=engine.FLAG_SYMMETRY_AVG)
    ref = _reference(eng, positions)
    eng.close()
    batch = -(-_row_limit_rows(384) // 8)
    eng = _big_engine(path, batch, engine.FLAG_SYMMETRY_AVG)
    idx = _slot_positions(batch)
    _run(eng, positions, idx)
    bad = _mismatches(eng, ref, idx)
    eng.close()
    assert not bad, "rows 8 s .. 8 s + 7 of slot s: " + _row_report(bad, _first_wrapped_row(384) // 8, "slots", 8)


_BLOCKW_CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import numpy as np
from p3achygo_amd import engine
from test_engine_gpu import _logits_close
path, pos_file, ref_file, rows, out = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5]
pos = np.load(pos_file)
ref = np.load(ref_file)
try:
    eng = engine.HipEngine(path, rows)
except engine.EngineError as err:
    json.dump({"skip": str(err)}, open(out, "w"))
    sys.exit(0)
idx = (7 * np.arange(rows) + rows) %% len(pos)
for s, p in enumerate(idx):
    eng.LoadBatch(s, pos[p:p + 1])
eng.RunInference()
bad = [s for s, p in enumerate(idx) if not _logits_close(eng.get_raw(s)[:1889], ref[p][:1889])]
eng.close()
json.dump({"bad": bad}, open(out, "w"))
"""


def test_hand_scheduled_block_kernel_rows_past_the_32_bit_element_offset(built, weight_files, positions, tmp_path):
    """k_blockw (P3HIP_BLOCKW=1, a child process) at C = 256 past the row limit, against the HIP kernels' reference
    of each position: the two differ by fp16 roundings, so within the logit bound"""
    from p3achygo_amd import engine
    path = weight_files("test_b3c256btl1")
    eng = engine.HipEngine(path, NPOS)
    _run(eng, positions, range(NPOS))
    ref = np.stack([eng.get_raw(s) for s in range(NPOS)])
    eng.close()
    np.save(tmp_path / "pos.npy", positions)
    np.save(tmp_path / "ref.npy", ref)
    env = dict(os.environ)
    for k in ("P3HIP_NO_BFUSE", "P3HIP_BLOCKW", "P3HIP_BLOCKW_DIAG"):
        env.pop(k, None)
    env["P3HIP_BLOCKW"] = "1"
    env["PYTHONPATH"] = os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
    rows = _row_limit_rows(256)
    out = str(tmp_path / "blockw.json")
    r = subprocess.run([sys.executable, "-c", _BLOCKW_CHILD % ROOT, path, str(tmp_path / "pos.npy"),
                        str(tmp_path / "ref.npy"), str(rows), out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.load(open(out))
    if "skip" in res:
        if "out of memory" in res["skip"].lower():
            pytest.skip("%d rows under P3HIP_BLOCKW=1: %s" % (rows, res["skip"]))
        pytest.fail(res["skip"])
    assert not res["bad"], _row_report(res["bad"], _first_wrapped_row(256))
