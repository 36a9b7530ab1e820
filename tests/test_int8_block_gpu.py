"""Fused INT8 blocks of the C = 256 btl trunks on the MI355X (P3HIP_FLAG_INT8_FUSED).

Every engine here is calibrated on tests/int8_restatement.calibration_batches() (or loads the scales of one that was).
Accuracy is judged against the float64 goldens within int8_block_restatement.BOUNDS, and block by block, teacher-forced,
against the CPU emulation of the same scheme (tests/int8_block_restatement.py) run from the engine's own x.

Measured on one MI355X (mean |d x| to the INT8 emulation over mean |d x| to the unquantized fp16 block, per btl block,
bound 0.5): see DESIGN.md section 9 "Fused INT8 blocks"."""
import hashlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT, load_golden  # noqa: E402
import int8_block_restatement as br  # noqa: E402
import int8_gpu_common as gc  # noqa: E402
import trunk_emulation as te  # noqa: E402

pytestmark = pytest.mark.gpu

BATCHES = (1, 7, 61, 1024)
BLOCK_JOBS = [("test_b3c256btl1", 1), ("test_b5c256btl2_i2", 37), ("test_b10c256btl1_i2", 37), ("b12c256btl3", 300)]
RATIO_BOUND = 0.5


_E = gc.Engines("FLAG_INT8_FUSED", raw_f64=True)
_flag, _calibrated, _scales, _with_scales, _fetch, _run = _E.flag, _E.calibrated, _E.scales, _E.with_scales, _E.fetch, _E.run
_weights, _oracle, _job_batch = gc.weights, gc.oracle_outputs, gc.job_batch


@pytest.mark.parametrize("name", br.SERVED)
def test_engine_matches_the_goldens_within_the_emulation_bounds_at_every_batch(built, weight_files, name):
    """Batches of 1, 7, 61 and 1024: the fixture's positions repeated to fill the batch; every copy within BOUNDS of the
    golden (so inside three times the emulation's own error) and bit-identical to the first copy."""
    g, pos = load_golden(name)
    path = weight_files(name)
    for batch in BATCHES:
        eng = _with_scales(path, batch)
        idx = np.arange(batch) % len(pos)
        eng.load_all(pos[idx])
        eng.RunInference()
        got = _fetch(eng, range(batch))
        eng.close()
        n = min(batch, len(pos))
        err = br.errors({k: v[:n] for k, v in got.items()}, {k: np.asarray(g[k])[:n] for k in got})
        print(f"{name} batch {batch}: {err}")
        for k, bound in br.BOUNDS[name].items():
            assert err[k] <= bound, (name, batch, err)
        for k in got:
            assert np.array_equal(got[k], got[k][idx]), (name, batch, k)   # copies of a position: bit-identical


_CHILD = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np
from p3achygo_amd import engine, features
d = np.load(sys.argv[1], allow_pickle=True)
out = {}
for key in d["keys"]:
    path, C, nblk, slots = d[key + ":path"].item(), int(d[key + ":C"]), int(d[key + ":blocks"]), d[key + ":slots"]
    pos = np.frombuffer(d[key + ":pos"].tobytes(), dtype=features.features_dtype()).copy()
    cal = np.frombuffer(d["cal"].tobytes(), dtype=features.features_dtype()).copy().reshape(int(d["ncal"]), -1)
    os.environ.pop("P3HIP_DEBUG_STOP_BLOCK", None)
    eng = engine.HipEngine(path, 16, flags=engine.FLAG_INT8_FUSED)
    for c in cal:
        eng.load_all(c)
        eng.int8_calibrate()
    scales = eng.int8_scales()
    eng.close()
    out[key + ":scales"] = scales
    for stop in range(nblk + 1):
        if stop < nblk:
            os.environ["P3HIP_DEBUG_STOP_BLOCK"] = str(stop)
        else:
            os.environ.pop("P3HIP_DEBUG_STOP_BLOCK", None)
        eng = engine.HipEngine(path, len(pos), flags=engine.FLAG_INT8_FUSED)
        eng.set_int8_scales(scales)
        eng.load_all(pos)
        eng.RunInference()
        out[f"{key}:x{stop}"] = eng.debug_x(len(pos), C)[slots]
        if stop == nblk:
            out[f"{key}:raw"] = np.stack([eng.get_raw(int(s)) for s in slots])
        eng.close()
np.savez(sys.argv[2], **out)
"""


@pytest.mark.parametrize("name,batch", BLOCK_JOBS)
def test_blocks_teacher_forced(built, tmp_path, name, batch):
    """One child process per configuration under its own time limit, nothing retried.  The engine's x after block k
    against the emulation of block k from the engine's x after block k - 1 with the engine's scales: for a btl block
    mean |d| to the INT8 emulation below 0.5 of mean |d| to the unquantized fp16 block; the stem, the broadcast blocks
    and the heads (the fp16 engine's kernels) by trunk_emulation's bounds."""
    import torch
    from p3achygo_amd import netspec
    cfg, W = _weights(name)
    path = str(tmp_path / (name + ".p3w"))
    netspec.save_p3w(path, cfg, W)
    pos, slots = _job_batch(name, batch)
    cal = np.stack(br.calibration_batches())
    spec = {"keys": np.array([name]), name + ":path": np.array(path), name + ":C": np.array(cfg.channels),
            name + ":blocks": np.array(cfg.blocks), name + ":slots": slots,
            name + ":pos": np.frombuffer(pos.tobytes(), np.uint8), "cal": np.frombuffer(cal.tobytes(), np.uint8),
            "ncal": np.array(len(cal))}
    inp, outp = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(inp, **spec)
    env = dict(os.environ)
    for k in ("P3HIP_NO_FUSE", "P3HIP_NO_BFUSE", "P3HIP_DEBUG_STOP_BLOCK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, str(inp), str(outp)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = np.load(outp)
    scales = out[name + ":scales"]
    assert len(scales) == len(br.quantized_tensors(cfg))
    xs = [out[f"{name}:x{s}"].astype(np.float64).reshape(len(slots), cfg.channels, 19, 19) for s in range(cfg.blocks + 1)]
    emu = te.Trunk(cfg, W)
    x0 = emu.stem(pos[slots])
    te.check_block(xs[0], x0, te.rms(x0), f"{name} stem", slots, *te.bounds(cfg, "stem"))
    worst = 0.0
    for k in range(cfg.blocks):
        if cfg.block_kind(k) == "broadcast":
            m = emu.block(k, torch.from_numpy(xs[k]))
            te.check_block(xs[k + 1], m, te.block_scale(xs[k], m), f"{name} block {k} (broadcast)", slots,
                           *te.bounds(cfg, k))
            continue
        q = br.block(cfg, W, k, xs[k], br.block_scales(cfg, scales, k))
        f = br.block(cfg, W, k, xs[k], None)
        d_q, d_f = float(np.abs(xs[k + 1] - q).mean()), float(np.abs(xs[k + 1] - f).mean())
        print(f"{name} batch {batch} block {k}: mean |d| to the INT8 emulation {d_q:.3e}, to the fp16 block {d_f:.3e}, "
              f"ratio {d_q / d_f:.3f}")
        worst = max(worst, d_q / d_f)
        assert np.isfinite(xs[k + 1]).all()
        assert d_q < RATIO_BOUND * d_f, (name, k, d_q, d_f)
    want = emu.heads(torch.from_numpy(xs[-1]))
    d = np.abs(out[f"{name}:raw"] - want)
    assert d.max() <= te.HEADS_TOL, (name, float(d.max()))
    print(f"{name}: worst btl ratio {worst:.3f}, heads max |d| {d.max():.2e}")


def test_engine_implements_the_emulated_scheme(built, weight_files):
    """test_b3c256btl1 (six quantized tensors), a ragged batch: mean |d logit| to the emulation with the engine's scales
    below half of that to float64."""
    from p3achygo_amd import features
    name = "test_b3c256btl1"
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
    emu = br.forward(cfg, W, planes, sc, scales=scales)
    d_emu = np.abs(got["raw"][:, :362] - emu["raw"][:, :362]).mean()
    d_f64 = np.abs(got["raw"][:, :362] - f64["raw"][:, :362]).mean()
    print(f"mean |d logit| to the emulation {d_emu:.3e}, to float64 {d_f64:.3e}")
    assert d_emu < 0.5 * d_f64, (d_emu, d_f64)


def test_peaked_policy_keeps_the_argmax(built, weight_files):
    """b12c256btl3_peaked (policy output layer x12): the engine's move argmax agrees with the float64 golden on no
    fewer positions than the emulation's, less one."""
    name = "b12c256btl3"
    g, pos = load_golden(name + "_peaked")
    path = weight_files(name, peak=12.0)
    cfg, W = _weights(name, peak=12.0)
    eng = _calibrated(path, 16)
    scales = eng.int8_scales()
    got = _run(eng, pos)
    eng.close()
    emu = br.forward(cfg, W, g["planes"], g["scalars"], scales=scales)
    am = lambda o: np.asarray(o["raw"])[:, :362].argmax(1)
    agree_eng = int((am(got) == am(g)).sum())
    agree_emu = int((am(emu) == am(g)).sum())
    print(f"argmax agreement with float64: engine {agree_eng}, emulation {agree_emu} of {len(pos)}")
    assert agree_eng >= agree_emu - 1, (agree_eng, agree_emu)


@pytest.mark.parametrize("name", ["test_b3c256btl1", "test_b5c256btl2_i2"])
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
    want = br.minmax_scales(cfg, W, [net.fill_inputs(c) for c in br.calibration_batches()])
    assert len(sa) == len(want) == len(br.quantized_tensors(cfg))
    # the engine calibrates on its fp16 plan: equal within a few fp16 roundings of the maxima
    np.testing.assert_allclose(sa, want, rtol=4e-3, atol=0)


def test_saved_scales_reproduce_the_results_and_bad_calls_fail(built, weight_files):
    from p3achygo_amd import engine, features
    path = weight_files("test_b5c256btl2_i2")
    pos = features.random_positions(24, seed=31)
    a = _calibrated(path, 32)
    want = _run(a, pos)["raw"]
    scales = a.int8_scales()
    a.close()
    b = engine.HipEngine(path, 32, flags=_flag())
    assert len(b.int8_scales()) == len(scales)
    b.LoadBatch(0, pos[:1])
    with pytest.raises(engine.EngineError, match="no activation scales"):
        b.RunInference()
    b.set_int8_scales(scales)
    assert np.array_equal(b.int8_scales(), scales)
    assert np.array_equal(_run(b, pos)["raw"], want)
    with pytest.raises(engine.EngineError, match="quantized tensors"):
        b.set_int8_scales(scales[:-1])
    b.close()


def test_launch_graph_replays_bit_for_bit_and_sees_new_scales(built, weight_files):
    from p3achygo_amd import engine, features
    path = weight_files("test_b5c256btl2_i2")
    B = 32
    pos = features.random_positions(B, seed=8)
    ref = _with_scales(path, B)
    gr = _with_scales(path, B, engine.FLAG_LAUNCH_GRAPH)
    s = ref.int8_scales()
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


def test_with_the_hbm_cache(built, weight_files):
    """Cache hits are bit-identical to the INT8_FUSED evaluation."""
    from p3achygo_amd import features
    path = weight_files("test_b3c256btl1")
    pos = features.random_positions(16, seed=12)
    ref = _with_scales(path, 16)
    want = _run(ref, pos)["raw"]
    ref.close()
    eng = _with_scales(path, 16)
    eng.EnableCache(8)
    key = lambda i: (1000 + i, 77)
    for rnd in range(2):
        for i in range(16):
            eng.LoadBatchKeyed(i, pos[i:i + 1], *key(i))
        eng.RunInference()
        for i in range(16):
            if rnd == 0:
                assert np.array_equal(eng.get_raw(i), want[i])
            r, _, hit = eng.GetBatchKeyed(i)
            assert hit == (rnd == 1)
            assert np.array_equal(np.ctypeslib.as_array(r.move_logits), want[i][:362].astype(np.float32))
    eng.close()


def test_symmetry_averaging_follows_the_rule_bit_for_bit(built, weight_files):
    from p3achygo_amd import engine, features
    from test_symmetry_avg_gpu import _check_rule
    path = weight_files("test_b3c256btl1")
    _check_rule(path, features.random_positions(19, seed=44), engine.symmetry_maps()[0], masks=(0x01, 0x81, 0xFF),
                flags=_flag(), scales=_scales(path))


def test_compaction_and_run_all_slots_equal_the_plain_engine(built, weight_files):
    from p3achygo_amd import engine, features
    path = weight_files("test_b10c256btl1_i2")
    pos = features.random_positions(20, seed=17)
    plain = _with_scales(path, 20)
    want = _run(plain, pos)["raw"]
    plain.close()
    slots = list(range(2, 62, 3))              # 20 of 64 slots: compacted to a dense batch of 20
    comp = _with_scales(path, 64)
    assert np.array_equal(_run(comp, pos, slots)["raw"], want)
    comp.close()
    allslots = _with_scales(path, 64, engine.FLAG_RUN_ALL_SLOTS)
    assert np.array_equal(_run(allslots, pos, slots)["raw"], want)
    allslots.close()


def test_repeated_and_concurrent_runs_are_bit_identical(built, weight_files):
    from p3achygo_amd import features
    path = weight_files("b12c256btl3")
    batch = 128
    pos = np.tile(features.random_positions(32, seed=2, n_games=8), batch // 32).copy()
    _scales(path)

    def digest(eng):
        h = hashlib.sha1()
        for s in (0, 1, batch // 2, batch - 1, 77):
            h.update(eng.get_raw(s).tobytes())
        return h.hexdigest()

    def worker(out, iters):
        eng = _with_scales(path, batch)
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


def test_trunk_kernel_timing_names_the_block_kernel(built, weight_files):
    from p3achygo_amd import features
    eng = _with_scales(weight_files("b12c256btl3"), 16)
    eng.load_all(features.random_positions(16, seed=3))
    eng.upload()
    ms, flops, kname = eng.time_trunk_kernel(16, 2)
    eng.close()
    assert kname == "k_block_i8<256,128>" and ms > 0
    assert flops == 2.0 * 16 * 361 * (3 * 9 * 128 * 128 + 2 * 256 * 128)
