"""Conv trunks of any width from 64 to 512 channels (netspec.WIDE_CONV_CONFIGS, csrc/conv_any.hip) on the HIP engine,
through the C ABI: parity with the float64 restatement (tests/trunk_emulation.py Trunk, fp16=False) at several batch
sizes, the zero padding of C and C_b, every block on its own against the fp16 emulation, the templated layer-wise
shapes through the same kernels bit for bit (P3HIP_CONV_ANY=1), compaction, RUN_ALL_SLOTS, launch-graph replay, the
NN cache and symmetry averaging, activation offsets past 2^31 elements, the timing hook and an evaluation match.

Tolerances, by the rule of tests/test_transformer_widths_gpu.py: the bounds of tests/test_engine_gpu.py (raw outputs
max(6e-3, 1e-3 |ref|), probabilities 5e-5, value probabilities 5e-4, KL 2e-6) where the fp16 emulation stays at or
below half of them, else twice the emulated error.  Emulated errors (16 positions, seed 11; the largest raw-output
error and its share of the raw-output bound, move / value / score / opt-move probabilities, largest KL):
    test_b3c64btl2        1.23e-3 0.20  2.1e-6  1.9e-4  2.2e-7  2.5e-6  8.2e-8
    test_b3c96nbt         1.51e-3 0.25  4.4e-6  1.4e-4  1.5e-6  5.3e-6  6.9e-8
    test_b3c192btl3       9.24e-4 0.15  2.5e-6  6.4e-5  4.2e-7  2.4e-6  2.9e-8
    test_b3c256btl2_cb64  1.05e-3 0.18  2.0e-6  1.4e-4  1.6e-7  3.3e-6  3.8e-8
    test_b3c128classic    1.05e-3 0.17  3.4e-6  1.1e-4  3.9e-7  4.2e-6  3.7e-8
    test_b3c320nbt        1.45e-3 0.24  3.5e-6  8.2e-5  8.0e-7  4.2e-6  3.8e-8
    test_b3c512nbt        1.44e-3 0.24  3.8e-6  1.3e-4  8.4e-7  3.2e-6  3.9e-8
    test_b4c512btl3_i2    1.30e-3 0.22  3.2e-6  7.7e-5  2.0e-7  4.2e-6  3.7e-8
    b12c192btl3           2.01e-3 0.34  7.4e-6  1.6e-4  6.6e-7  1.1e-5  1.1e-7
    b10c512nbt            4.59e-3 0.77  4.2e-5  3.9e-4  2.3e-6  7.2e-5  5.9e-7
So every net takes the bounds of tests/test_engine_gpu.py, but b10c512nbt: raw outputs 9.2e-3, move probabilities
8.4e-5, value probabilities 7.8e-4, opt-move probabilities 1.45e-4 (score probabilities and KL as the others).
tests/test_conv_widths_cpu.py re-measures the table and checks it stays at or below half of every bound here.

Block by block (test_b3c320nbt, test_b4c512btl3_i2, test_b3c128classic): trunk_emulation.BOUNDS "stem", "lw_btl",
"lw_nbt", "classic" and "broadcast".  The twin on these nets (tests/test_conv_widths_cpu.py, the 37-position batch):
worst error / lowest identical fraction lw_nbt 3.31 / 0.513, lw_btl 0.95 / 0.804, classic 1.70 / 0.641, broadcast
0.90 / 0.891, stem 0.81 / 1.000 — inside half of every bound and above every fraction, so no net changes a bound.

No figure of an MI355X is recorded here yet: when this file was written it had not run on one.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_widths_common as cw  # noqa: E402
from conftest import ROOT  # noqa: E402

pytestmark = pytest.mark.gpu

# the emulation's errors as measured on the CPU (module docstring), rounded up in the third digit
_COLS = ("logit", "logit_share", "move_probs", "value_probs", "score_probs", "opt_move_probs", "kl")
EMULATED = {n: dict(zip(_COLS, v)) for n, v in {
    "test_b3c64btl2": (0.00123, 0.205, 2.1e-06, 0.000191, 2.23e-07, 2.48e-06, 8.21e-08),
    "test_b3c96nbt": (0.00152, 0.252, 4.43e-06, 0.000143, 1.46e-06, 5.28e-06, 6.87e-08),
    "test_b3c192btl3": (0.000925, 0.155, 2.53e-06, 6.45e-05, 4.24e-07, 2.38e-06, 2.88e-08),
    "test_b3c256btl2_cb64": (0.00105, 0.175, 2.05e-06, 0.000137, 1.64e-07, 3.29e-06, 3.84e-08),
    "test_b3c128classic": (0.00105, 0.175, 3.39e-06, 0.000107, 3.93e-07, 4.17e-06, 3.66e-08),
    "test_b3c320nbt": (0.00145, 0.242, 3.46e-06, 8.21e-05, 8.02e-07, 4.17e-06, 3.79e-08),
    "test_b3c512nbt": (0.00144, 0.24, 3.78e-06, 0.000133, 8.42e-07, 3.19e-06, 3.85e-08),
    "test_b4c512btl3_i2": (0.00131, 0.217, 3.18e-06, 7.65e-05, 2.05e-07, 4.18e-06, 3.71e-08),
    "b12c192btl3": (0.00201, 0.335, 7.4e-06, 0.000162, 6.63e-07, 1.1e-05, 1.06e-07),
    "b10c512nbt": (0.00459, 0.765, 4.17e-05, 0.000386, 2.31e-06, 7.23e-05, 5.92e-07),
}.items()}
TOL = {n: cw.tolerance(e) for n, e in EMULATED.items()}
# (bounds of the block checker that a twin's measurement changed: none, module docstring)
BLOCK_BOUNDS = {n: {} for n in cw.BLOCK_NETS}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> .p3w of netspec.generate_weights(cfg, randomize=True), written on demand"""
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("conv_widths")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = os.path.join(d, name + ".p3w")
            netspec.save_p3w(cache[name], cw.config(name), cw.weights(name))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def reference():
    """name -> (positions, float64 outputs of them), computed once per net"""
    cache = {}

    def get(name):
        if name not in cache:
            pos = cw.positions()
            cache[name] = (pos, cw.outputs(cw.config(name), cw.weights(name), pos, fp16=False))
        return cache[name]
    return get


def _raws(eng, slots):
    return [eng.get_raw(s).copy() for s in slots]


@pytest.mark.parametrize("name", cw.NETS)
def test_engine_matches_the_restatement_at_batch_sizes(built, files, reference, name):
    """batch 1, 7, 61 and 1024; slot s holds reference position (7 s + batch) mod 16; slots holding the same position
    are bit-identical across slots and batch sizes"""
    from p3achygo_amd import engine, netspec
    pos, ref = reference(name)
    n = len(pos)
    seen = {}
    for batch in (1, 7, 61, 1024):
        idx = (7 * np.arange(batch) + batch) % n
        eng = engine.HipEngine(files(name), batch)
        eng.load_all(pos[idx])
        eng.RunInference()
        raws = np.stack(_raws(eng, range(batch)))
        for s in range(batch):
            i = int(idx[s])
            if i not in seen:
                seen[i] = raws[s].copy()
            assert np.array_equal(raws[s], seen[i]), (name, batch, s)
            if s < 64 or s % 37 == 0:   # the record of every distinct position at every batch, and a sample beyond
                cw.check_outputs(name, TOL[name], raws[s], eng.GetBatch(s), ref, i)
                own = eng.GetOwnership(s)
                assert np.abs(own - ref["raw"][i][1526:1887]).max() <= TOL[name]["logit"]
                assert np.array_equal(own, raws[s][1526:1887])
        if batch == 1024:
            t, c3 = eng.flops_per_position()
            want_t, want_c3 = netspec.flops_per_position(cw.config(name))
            assert abs(t - want_t) < 1.0 and abs(c3 - want_c3) < 1.0   # the file's widths, not the padded ones
        eng.close()


@pytest.mark.parametrize("name", cw.PADDED_NETS)
def test_padded_channels_of_the_stream_are_exactly_zero(built, files, reference, name):
    from p3achygo_amd import engine
    C = cw.config(name).channels
    Cp = cw.padded(C)
    pos, _ = reference(name)
    eng = engine.HipEngine(files(name), len(pos))
    eng.load_all(pos)
    eng.RunInference()
    x = eng.debug_x(len(pos), Cp)   # p3hip_debug_x returns the padded width
    assert np.all(x[:, C:] == 0)
    assert (np.abs(x[:, :C]).max(axis=(0, 2)) > 0).all()
    eng.close()


def _engine_xs(path, cfg, pos, slots):
    """x after the stem and after every block (P3HIP_DEBUG_STOP_BLOCK, read at create), cut to the file's C"""
    from p3achygo_amd import engine
    C, Cp = cfg.channels, cw.padded(cfg.channels)
    old = os.environ.get("P3HIP_DEBUG_STOP_BLOCK")
    xs = []
    try:
        for stop in range(cfg.blocks + 1):
            os.environ["P3HIP_DEBUG_STOP_BLOCK"] = str(stop)
            eng = engine.HipEngine(path, len(pos))
            eng.load_all(pos)
            eng.RunInference()
            xs.append(eng.debug_x(len(pos), Cp)[slots][:, :C])
            eng.close()
    finally:
        if old is None:
            os.environ.pop("P3HIP_DEBUG_STOP_BLOCK", None)
        else:
            os.environ["P3HIP_DEBUG_STOP_BLOCK"] = old
    return xs


def block_batch(batch):
    """positions of a block-by-block job and the slots compared (all of them up to 37, a strided sample beyond)"""
    from p3achygo_amd import features
    pos = features.random_positions(batch, seed=43, n_games=16, max_moves=300, komis=(7.5, -7.5, 0.5))
    slots = np.arange(batch) if batch <= 37 else np.asarray(sorted(set(range(5, batch, 29)) | {0, batch - 1}))
    return pos, slots


@pytest.mark.parametrize("name", cw.BLOCK_NETS)
def test_blocks_teacher_forced(built, files, name):
    """the stem and every block from the engine's own x before it, inside trunk_emulation's layer-wise bounds"""
    cfg, W = cw.config(name), cw.weights(name)
    for batch in (1, 37, 300):
        pos, slots = block_batch(batch)
        xs = _engine_xs(files(name), cfg, pos, slots)
        st = cw.teacher_forced(cw.trunk(cfg, W), xs, pos[slots], slots=slots, label=f"{name} batch {batch} block ",
                               bounds=BLOCK_BOUNDS[name])
        print(name, batch, {k: (round(v["max_err"], 2), round(v["identical"], 3)) for k, v in st.items()})


_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from p3achygo_amd import engine, features
out = {}
for spec in sys.argv[2:]:
    name, path = spec.split("=", 1)
    for batch in (37, 300):
        pos = features.random_positions(batch, seed=43)
        eng = engine.HipEngine(path, batch)
        eng.load_all(pos)
        eng.RunInference()
        out["%%s:%%d" %% (name, batch)] = np.stack([eng.get_raw(s) for s in range(batch)])
        eng.close()
np.savez(sys.argv[1], **out)
"""


def test_templated_shapes_through_the_runtime_width_kernels_bit_for_bit(built, weight_files, tmp_path):
    """P3HIP_CONV_ANY=1 (read at p3hip_create) sends C = 384 / C_b = 192 btl and nbt and classic C = 192 through
    conv_any.hip: the same slices in the same order, so the raw outputs are those of the templated kernels"""
    names = ["test_b3c384btl3", "test_b3c384nbt", "test_b3c192classic"]
    specs = ["%s=%s" % (n, weight_files(n)) for n in names]
    got = {}
    for label, val in (("default", None), ("any", "1")):
        env = dict(os.environ)
        env.pop("P3HIP_CONV_ANY", None)
        if val:
            env["P3HIP_CONV_ANY"] = val
        outp = tmp_path / (label + ".npz")
        r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, str(outp)] + specs, env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        got[label] = np.load(outp)
    for k in got["default"].files:
        a, b = got["default"][k], got["any"][k]
        assert np.abs(a).max() > 0 and not np.isnan(a).any()
        assert a.tobytes() == b.tobytes(), (k, np.argwhere(a != b)[:5])


@pytest.mark.parametrize("name", cw.PATH_NETS)
def test_compaction_and_run_all_slots(built, files, reference, name):
    from p3achygo_amd import engine
    pos, ref = reference(name)
    eng = engine.HipEngine(files(name), 40)
    for s in range(32):
        eng.LoadBatch(s, pos[s % 16:s % 16 + 1])
    eng.RunInference()
    full = _raws(eng, range(32))
    part = [2, 9, 10, 31]
    for s in part:
        eng.LoadBatch(s, pos[s % 16:s % 16 + 1])
    eng.RunInference()
    assert all(np.array_equal(a, full[s]) for a, s in zip(_raws(eng, part), part))
    eng.close()
    eng = engine.HipEngine(files(name), 8, flags=engine.FLAG_RUN_ALL_SLOTS)
    eng.LoadBatch(5, pos[5:6])
    eng.RunInference()
    assert np.array_equal(eng.get_raw(5), full[5])
    cw.check_outputs(name, TOL[name], eng.get_raw(5), eng.GetBatch(5), ref, 5)
    eng.GetBatch(0)                                      # every slot of the static batch was run
    eng.close()


@pytest.mark.parametrize("name", cw.PATH_NETS)
def test_launch_graph_replays_bit_for_bit(built, files, reference, name):
    from p3achygo_amd import engine
    pos, _ = reference(name)
    B = 48
    tiled = pos[np.arange(B) % 16]
    ref = engine.HipEngine(files(name), B)
    gr = engine.HipEngine(files(name), B, flags=engine.FLAG_LAUNCH_GRAPH)
    ref.load_all(tiled)
    ref.RunInference()
    want = _raws(ref, range(B))
    for rnd in range(4):                       # eager, capture, replay, replay
        gr.load_all(tiled)
        gr.RunInference()
        assert all(np.array_equal(a, b) for a, b in zip(want, _raws(gr, range(B)))), rnd
        assert gr.graph_state() == (1 if rnd >= 1 else 0)
    ref.close()
    gr.close()


@pytest.mark.parametrize("name", cw.PATH_NETS)
def test_nn_cache_hits_are_bit_identical(built, files, reference, name):
    from p3achygo_amd import engine
    pos, _ = reference(name)
    key = lambda i: (0x9E3779B97F4A7C15 * (i + 1) & (2**64 - 1), 0xC2B2AE3D27D4EB4F * (i + 7) & (2**64 - 1))
    eng = engine.HipEngine(files(name), 16)
    eng.EnableCache(8)
    for s in range(16):
        eng.LoadBatchKeyed(s, pos[s:s + 1], *key(s), symmetry=s % 8)
    eng.RunInference()
    want = _raws(eng, range(16))
    for s in range(16):
        k = 15 - s
        eng.LoadBatchKeyed(s, pos[(k + 5) % 16:(k + 5) % 16 + 1], *key(k), symmetry=1)
    eng.RunInference()
    for s in range(16):
        _, sym, hit = eng.GetBatchKeyed(s)
        assert hit and sym == (15 - s) % 8 and np.array_equal(eng.get_raw(s), want[15 - s])
    eng.close()


@pytest.mark.parametrize("name", cw.PATH_NETS)
def test_symmetry_averaging_is_the_restated_reduce(built, files, name):
    """the k-copy reduce of tests/symavg_restatement.py over a plain engine's copies, bit for bit"""
    from p3achygo_amd import engine, features
    from test_symmetry_avg_gpu import _check_rule
    _check_rule(files(name), features.random_positions(21, seed=47), engine.symmetry_maps()[0], masks=(0x01, 0x81, 0xFF))


def test_activation_offsets_past_2_31_elements_c512(built, files):
    """12,288 rows of 512 x 361 activations: 2.27e9 elements; the element offset of a row passes 2^31 from row index
    11,619 on (the 11,620th row: 2^31 / (512 x 361) = 11,618.6); every slot bit-identical to a 61-position run of the
    same position"""
    from p3achygo_amd import engine, features
    name, npos, rows = "test_b3c512nbt", 61, 12288
    assert rows * 512 * 361 > 11619 * 512 * 361 > 2 ** 31 > 11618 * 512 * 361
    pos = features.random_positions(npos, seed=61, n_games=41, max_moves=330, komis=(7.5, -7.5, 0.5))

    def out(eng, s):
        r = eng.GetBatch(s)
        return np.concatenate([eng.get_raw(s), np.ctypeslib.as_array(r.move_probs),
                               np.ctypeslib.as_array(r.value_probs)]).astype(np.float32).view(np.uint32)
    eng = engine.HipEngine(files(name), npos)
    eng.load_all(pos)
    eng.RunInference()
    ref = [out(eng, s) for s in range(npos)]
    eng.close()
    eng = engine.HipEngine(files(name), rows)
    idx = (7 * np.arange(rows) + rows) % npos
    eng.load_all(pos[idx])
    eng.RunInference()
    bad = [s for s in range(rows) if not np.array_equal(out(eng, s), ref[idx[s]])]
    eng.close()
    assert not bad, (len(bad), bad[:8], [b for b in bad if b >= 11619][:8])


@pytest.mark.parametrize("name", cw.PATH_NETS + ["test_b3c128classic"])
def test_trunk_kernel_timing_names_the_runtime_width_conv(built, files, reference, name):
    from p3achygo_amd import engine
    pos, _ = reference(name)
    cfg = cw.config(name)
    w3 = cfg.channels if cfg.block_type == "classic" else cfg.bottleneck_channels   # the file's width, unpadded
    eng = engine.HipEngine(files(name), 64)
    eng.load_all(pos[np.arange(64) % 16])
    eng.upload()
    ms, fl, kname = eng.time_trunk_kernel(64, 2)
    assert ms > 0 and kname == "k_lconv_any<3>" and fl == 2.0 * 9 * w3 * w3 * 361 * 64
    eng.close()


def test_eval_match_between_two_new_shapes(built, files):
    from p3achygo_amd import host_api
    st = host_api.eval_match(files("b12c192btl3"), files("test_b3c320nbt"), num_games=4, visits_per_move=16,
                             leaves_per_round=4, max_moves=24, num_threads=2, seed=2)
    assert st.games == 4 and st.cur_wins + st.cand_wins + st.draws == 4
