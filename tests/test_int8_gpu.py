"""Calibrated INT8 inference of the layer-wise trunks on the MI355X (P3HIP_FLAG_INT8).

Every INT8 engine here is calibrated on tests/int8_restatement.calibration_batches() (seeded random positions, apart
from every evaluated set).  Accuracy is judged against the CPU emulation of the same scheme (tests/int8_restatement.py)
and the float64 goldens, within bounds derived from the emulation's own error (int8_restatement.BOUNDS)."""
import hashlib
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden  # noqa: E402
import int8_gpu_common as gc  # noqa: E402
import int8_restatement as ir  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = ("test_b3c384btl3", "test_b3c384nbt", "test_b3c192classic", "b14c384btl3", "b10c384nbt")


_E = gc.Engines("FLAG_INT8", raw_f64=True)
_calibrated, _run = _E.calibrated, _E.run
_weights, _oracle = gc.weights, gc.oracle_outputs


@pytest.mark.parametrize("name", GOLDEN)
def test_int8_engine_matches_the_goldens_within_the_emulation_bounds(built, weight_files, name):
    g, pos = load_golden(name)
    eng = _calibrated(weight_files(name), 16)
    got = _run(eng, pos)
    eng.close()
    err = ir.errors(got, g)
    for k, bound in ir.BOUNDS[name].items():
        assert err[k] <= bound, (name, err)


def test_int8_engine_implements_the_emulated_scheme(built, weight_files):
    """A ragged batch of random positions: the engine, run with its own calibrated scales, lands clearly closer to the
    INT8 emulation with those scales than to the float64 network (mean |d logit| less than half), so the kernels
    compute this quantization scheme, not merely something near fp16.  On the classic test net (four quantized tensors)
    the rounding flips that tiny differences cause stay few; deeper nets cascade them."""
    from p3achygo_amd import features
    name = "test_b3c192classic"
    path = weight_files(name)
    cfg, W = _weights(name)
    pos = features.random_positions(40, seed=4242, n_games=10)
    slots = list(range(3, 3 * 40 + 3, 3))    # scattered over a batch of 128
    eng = _calibrated(path, 128)
    scales = eng.int8_scales()
    got = _run(eng, pos, slots)
    eng.close()
    net, f64 = _oracle(path, pos)
    planes, sc = net.fill_inputs(pos)
    emu = ir.forward(cfg, W, planes, sc, scales=scales)
    d_emu = np.abs(got["raw"][:, :362] - emu["raw"][:, :362]).mean()
    d_f64 = np.abs(got["raw"][:, :362] - f64["raw"][:, :362]).mean()
    assert d_emu < 0.5 * d_f64, (d_emu, d_f64)


def test_int8_peaked_policy_keeps_the_argmax(built, weight_files):
    """The `_peaked` variant of b14c384btl3 (policy output layer x12): the INT8 engine's move argmax agrees with the
    float64 network on no fewer positions than the emulation's, less one."""
    from p3achygo_amd import features
    name = "b14c384btl3"
    path = weight_files(name, peak=12.0)
    cfg, W = _weights(name, peak=12.0)
    pos = features.random_positions(32, seed=515, n_games=8)
    eng = _calibrated(path, 32)
    scales = eng.int8_scales()
    got = _run(eng, pos)
    eng.close()
    net, f64 = _oracle(path, pos)
    planes, sc = net.fill_inputs(pos)
    emu = ir.forward(cfg, W, planes, sc, scales=scales)
    am = lambda o: o["raw"][:, :362].argmax(1)
    agree_eng = int((am(got) == am(f64)).sum())
    agree_emu = int((am(emu) == am(f64)).sum())
    assert agree_eng >= agree_emu - 1, (agree_eng, agree_emu)


@pytest.mark.parametrize("name", ["test_b3c384btl3", "test_b3c192classic"])
def test_calibrated_scales_match_the_emulation_and_repeat_bit_for_bit(built, weight_files, name):
    from oracle import oracle
    path = weight_files(name)
    cfg, W = _weights(name)
    a = _calibrated(path, 16)
    sa = a.int8_scales()
    a.close()
    b = _calibrated(path, 16)
    sb = b.int8_scales()
    b.close()
    assert np.array_equal(sa, sb)
    net = oracle.OracleNet(path)
    want = ir.minmax_scales(cfg, W, [net.fill_inputs(c) for c in ir.calibration_batches()])
    assert len(sa) == len(want) == len(ir.quantized_tensors(cfg))
    # the engine calibrates on its fp16 plan: equal within a few fp16 roundings of the maxima
    np.testing.assert_allclose(sa, want, rtol=4e-3, atol=0)


def test_saved_scales_reproduce_the_results_bit_for_bit(built, weight_files):
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c384nbt")
    pos = features.random_positions(24, seed=31)
    a = _calibrated(path, 32)
    want = _run(a, pos)["raw"]
    scales = a.int8_scales()
    a.close()
    b = engine.HipEngine(path, 32, flags=engine.FLAG_INT8)
    b.set_int8_scales(scales)
    assert np.array_equal(b.int8_scales(), scales)
    assert np.array_equal(_run(b, pos)["raw"], want)
    with pytest.raises(engine.EngineError, match="quantized tensors"):
        b.set_int8_scales(scales[:-1])
    b.close()


def test_uncalibrated_run_fails_and_other_trunks_are_refused(built, weight_files, tmp_path):
    from p3achygo_amd import engine, features, netspec
    import tfm_restatement
    eng = engine.HipEngine(weight_files("test_b3c192classic"), 8, flags=engine.FLAG_INT8)
    assert len(eng.int8_scales()) == len(ir.quantized_tensors(netspec.CONFIGS["test_b3c192classic"]))
    eng.LoadBatch(0, features.random_positions(1, seed=5))
    with pytest.raises(engine.EngineError, match="no activation scales"):
        eng.RunInference()
    eng.close()
    for name in ("b12c256btl3", "test_b3c128btl2"):
        with pytest.raises(engine.EngineError, match="INT8 is available only for layer-wise trunks"):
            engine.HipEngine(weight_files(name), 8, flags=engine.FLAG_INT8)
    cfg, W = tfm_restatement.fixture_weights("test_b2d96h3_tfm")
    p = str(tmp_path / "tfm.p3w")
    netspec.save_p3w(p, cfg, W)
    with pytest.raises(engine.EngineError, match="INT8 is available only for layer-wise trunks"):
        engine.HipEngine(p, 8, flags=engine.FLAG_INT8)
    engine.HipEngine(p, 8).close()   # the same file without the flag is served


def test_int8_launch_graph_replays_bit_for_bit_and_sees_new_scales(built, weight_files):
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c384btl3")
    B = 32
    pos = features.random_positions(B, seed=8)
    ref = _calibrated(path, B)
    gr = engine.HipEngine(path, B, flags=engine.FLAG_INT8 | engine.FLAG_LAUNCH_GRAPH)
    s = ref.int8_scales()
    gr.set_int8_scales(s)
    want = _run(ref, pos)["raw"]
    for rnd in range(4):                       # eager, capture, replay, replay
        assert np.array_equal(_run(gr, pos)["raw"], want), rnd
    assert gr.graph_state() == 1
    s2 = (s * np.float32(1.25)).astype(np.float32)
    ref.set_int8_scales(s2)
    gr.set_int8_scales(s2)
    want2 = _run(ref, pos)["raw"]
    assert not np.array_equal(want2, want)
    assert np.array_equal(_run(gr, pos)["raw"], want2) and gr.graph_state() == 1
    ref.close()
    gr.close()


def test_int8_with_the_hbm_cache(built, weight_files):
    """Cache hits are bit-identical to the INT8 evaluation; a calibration run on a cached engine evaluates every slot
    and stores nothing."""
    from p3achygo_amd import engine, features
    path = weight_files("test_b3c192classic")
    pos = features.random_positions(16, seed=12)
    ref = _calibrated(path, 16)
    want = _run(ref, pos)["raw"]
    eng = engine.HipEngine(path, 16, flags=engine.FLAG_INT8)
    eng.EnableCache(8)
    key = lambda i: (1000 + i, 77)
    cal = ir.calibration_batches()
    for c in cal:
        for i in range(len(c)):
            eng.LoadBatchKeyed(i, c[i:i + 1], *key(i))
        eng.int8_calibrate()
        for i in range(len(c)):
            _, _, hit = eng.GetBatchKeyed(i)
            assert not hit
    assert eng.cache_stats()["stored"] == 0 and eng.cache_stats()["lookups"] == 0
    assert np.array_equal(eng.int8_scales(), ref.int8_scales())
    for rnd in range(2):
        for i in range(16):
            eng.LoadBatchKeyed(i, pos[i:i + 1], *key(i))
        eng.RunInference()
        for i in range(16):
            assert np.array_equal(eng.get_raw(i), want[i]) if rnd == 0 else True
            r, _, hit = eng.GetBatchKeyed(i)
            assert hit == (rnd == 1)
            assert np.array_equal(np.ctypeslib.as_array(r.move_logits), want[i][:362].astype(np.float32))
    ref.close()
    eng.close()


def test_int8_repeated_and_concurrent_runs_are_bit_identical(built, weight_files):
    from p3achygo_amd import features
    path = weight_files("b10c384nbt")
    batch = 128
    pos = np.tile(features.random_positions(32, seed=2, n_games=8), batch // 32).copy()
    scales = []

    def digest(eng):
        h = hashlib.sha1()
        for s in (0, 1, batch // 2, batch - 1, 77):
            h.update(eng.get_raw(s).tobytes())
        return h.hexdigest()

    def worker(out, iters):
        eng = _calibrated(path, batch)
        scales.append(eng.int8_scales())
        ds = set()
        for _ in range(iters):
            eng.load_all(pos)
            eng.RunInference()
            ds.add(digest(eng))
        eng.close()
        out.append(ds)

    solo = []
    worker(solo, 6)
    assert len(solo[0]) == 1
    outs = []
    ths = [threading.Thread(target=worker, args=(outs, 6)) for _ in range(2)]
    [t.start() for t in ths]; [t.join() for t in ths]
    assert len(outs) == 2 and outs[0] == outs[1] == solo[0]
    assert all(np.array_equal(s, scales[0]) for s in scales)


def test_int8_trunk_kernel_timing_names_the_int8_kernel(built, weight_files):
    from p3achygo_amd import features
    eng = _calibrated(weight_files("test_b3c384btl3"), 16)
    eng.load_all(features.random_positions(16, seed=3))
    eng.upload()
    ms, flops, kname = eng.time_trunk_kernel(16, 2)
    eng.close()
    assert kname == "k_lconv_i8<3,192,192>" and ms > 0 and flops == 2.0 * 16 * 361 * 9 * 192 * 192
