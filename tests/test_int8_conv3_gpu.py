"""Calibrated INT8 for the 3x3 convs only on the MI355X (P3HIP_FLAG_INT8_CONV3, DESIGN.md section 9 "INT8 for the 3x3
convs only").

Every engine here is calibrated on tests/int8_restatement.calibration_batches() (or loads the scales of one that was).
The nets (int8_conv3_restatement.NETS) are three blocks each: the templated shapes with three passes of the reduce, the
nbt dual / res flows at both ends of the pairs, a runtime width with C_b padded, both widths padded, and one K slice with
one output pass (no prefetch); two classic nets for the equality with the existing INT8 plans.

Accuracy: block by block, teacher-forced, against the CPU emulation of the same scheme run from the engine's own x and with
the engine's own scales (mean |d| to the emulation below RATIO_BOUND of the mean |d| between that emulation and the
unquantized fp16 block), at batch 3 and at the first batch at which a workgroup of the fp16 1x1 reduce takes a second
position on this device; the whole net against the float64 outputs within int8_conv3_restatement.BOUNDS.  Everything else
is bit for bit: both kernel forms, the classic nets' existing plans, garbage in the padded weight channels, the scales
against an engine that quantizes every conv, saved scales, graph replay, compaction, RUN_ALL_SLOTS, repeats, the cache,
AUX.

Measured on one MI355X (256 CUs; test_blocks_teacher_forced, the ratio per layer-wise block, bound 0.5): 0.000 - 0.127 on
the btl nets, 0.005 - 0.311 on the nbt nets (the largest: the second block of test_b3c384nbt at batch 169); heads max |d|
1.8e-6.  Whole nets, largest move-logit error to float64: 0.005 (test_b3c64btl2) to 0.021 (test_b3c96nbt), 0.25 - 0.32 of
the bounds."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_widths_common as cw  # noqa: E402
import int8_any_restatement as ar  # noqa: E402
import int8_conv3_restatement as c3  # noqa: E402
import int8_gpu_common as gc  # noqa: E402
import trunk_emulation as te  # noqa: E402

pytestmark = pytest.mark.gpu

RATIO_BOUND = 0.5          # tests/test_int8_block_gpu.py, tests/test_int8_any_gpu.py
MECH_NET = "test_b3c96nbt"
CHILD_TIMEOUT = 240
HIP_ATTR_MULTIPROCESSOR_COUNT = 63         # hipDeviceAttributeMultiprocessorCount (hip/hip_runtime_api.h)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> .p3w of netspec.generate_weights(cfg, randomize=True); garbage=True: its zero-padded twin with garbage in
    the padded weight channels (_garbage_twin)"""
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("int8_conv3")
    cache = {}

    def get(name, garbage=False):
        key = (name, garbage)
        if key not in cache:
            cfg, W = c3.config(name), c3.weights(name)
            if garbage:
                cfg, W = _garbage_twin(cfg, W)
            cache[key] = os.path.join(d, name + ("_garbage" if garbage else "") + ".p3w")
            netspec.save_p3w(cache[key], cfg, W)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def n_cu(built):
    """CU count of device 0 as the engine's launchers see it, read from the HIP runtime libp3hip.so has loaded
    (tests/test_batch_geometry_gpu.py)"""
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


def second_position_batch(cfg, n_cu):
    """The first batch at which a workgroup of the fp16 1x1 reduce (k_lconv_q8: the launch with the quantizing epilogue)
    takes a second position: launch_util.h conv_split_grid with two workgroups per CU gives a grid of at most
    floor(2 n_cu / (8 ncp)) 8 ncp workgroups (at least 8 ncp), ncp = padded C_b / 64 output passes, so grid / ncp position
    groups.  The expand's ncp is larger, so its workgroups take a second position from a smaller batch on."""
    ncp = cw.padded(cfg.bottleneck_channels) // 64
    unit = 8 * ncp
    cap = max((2 * n_cu // unit) * unit, unit)
    return cap // ncp + 1


_E = gc.Engines("FLAG_INT8_CONV3", raw_f64=False)
_flag, _calibrated, _scales, _with_scales, _fetch, _run = _E.flag, _E.calibrated, _E.scales, _E.with_scales, _E.fetch, _E.run

_FAILED = []


def _child(script, args, env_extra=None):
    gc.child(script, args, _FAILED, CHILD_TIMEOUT, env_extra)


# ---- 1. blocks, teacher-forced ---------------------------------------------------------------------------------------

_BLOCKS_CHILD = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np
from p3achygo_amd import engine, features
d = np.load(sys.argv[1], allow_pickle=True)
path, Cp, nblk, slots = d["path"].item(), int(d["Cp"]), int(d["blocks"]), d["slots"]
pos = np.frombuffer(d["pos"].tobytes(), dtype=features.features_dtype()).copy()
cal = np.frombuffer(d["cal"].tobytes(), dtype=features.features_dtype()).copy().reshape(int(d["ncal"]), -1)
out = {}
os.environ.pop("P3HIP_DEBUG_STOP_BLOCK", None)
eng = engine.HipEngine(path, 16, flags=engine.FLAG_INT8_CONV3)
for c in cal:
    eng.load_all(c)
    eng.int8_calibrate()
scales = eng.int8_scales()
eng.close()
out["scales"] = scales
for stop in range(nblk + 1):
    if stop < nblk:
        os.environ["P3HIP_DEBUG_STOP_BLOCK"] = str(stop)
    else:
        os.environ.pop("P3HIP_DEBUG_STOP_BLOCK", None)
    eng = engine.HipEngine(path, len(pos), flags=engine.FLAG_INT8_CONV3)
    eng.set_int8_scales(scales)
    eng.load_all(pos)
    eng.RunInference()
    out["x%%d" %% stop] = eng.debug_x(len(pos), Cp)[slots]
    if stop == nblk:
        out["raw"] = np.stack([eng.get_raw(int(s)) for s in slots])
    eng.close()
# the fp16 engine's stem
os.environ["P3HIP_DEBUG_STOP_BLOCK"] = "0"
eng = engine.HipEngine(path, len(pos))
eng.load_all(pos)
eng.RunInference()
out["x0_fp16"] = eng.debug_x(len(pos), Cp)[slots]
eng.close()
np.savez(sys.argv[2], **out)
"""


@pytest.mark.parametrize("second", [False, True], ids=["batch3", "second_position"])
@pytest.mark.parametrize("name", c3.NETS)
def test_blocks_teacher_forced(built, files, tmp_path, n_cu, name, second):
    """The engine's x after block k against the emulation of block k from the engine's x after block k - 1 with the
    engine's scales: mean |d| to the emulation below 0.5 of the mean |d| between that emulation and the unquantized fp16
    block.  Where block k - 1 is layer-wise too the block's first conv, an fp16 1x1, read the fp16 activated copy of a sum
    the engine does not store: both emulations take int8_any_restatement.handed_on's estimate of it.  The stem, the
    broadcast block and the heads (the fp16 engine's kernels) by trunk_emulation's bounds, the stem bit for bit the fp16
    engine's; padded channels of the stream are exactly 0."""
    import torch
    from test_conv_widths_gpu import block_batch
    cfg, W = c3.config(name), c3.weights(name)
    C, Cp = cfg.channels, cw.padded(cfg.channels)
    batch = second_position_batch(cfg, n_cu) if second else 3
    pos, slots = block_batch(batch)
    cal = np.stack(c3.calibration_batches())
    inp, outp = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(inp, path=np.array(files(name)), Cp=np.array(Cp), blocks=np.array(cfg.blocks), slots=slots,
             pos=np.frombuffer(pos.tobytes(), np.uint8), cal=np.frombuffer(cal.tobytes(), np.uint8), ncal=np.array(len(cal)))
    _child(_BLOCKS_CHILD, [inp, outp])
    out = np.load(outp)
    scales = out["scales"]
    assert len(scales) == len(c3.quantized_tensors(cfg)) and (scales > 0).all()
    full = [out[f"x{s}"] for s in range(cfg.blocks + 1)]
    assert np.abs(full[0]).max() > 0
    assert out["x0_fp16"].tobytes() == full[0].tobytes()
    for x in full:
        assert np.isfinite(x).all() and np.all(x[:, C:] == 0)
    xs = [x[:, :C].astype(np.float64).reshape(len(slots), C, 19, 19) for x in full]
    emu = cw.trunk(cfg, W)
    x0 = emu.stem(pos[slots])
    te.check_block(xs[0], x0, te.rms(x0), f"{name} stem", slots, *te.BOUNDS["stem"])
    xa = None   # the estimate of the sum handed on
    worst = 0.0
    for k in range(cfg.blocks):
        if cfg.block_kind(k) == "broadcast":
            m = emu.block(k, torch.from_numpy(xs[k]))
            te.check_block(xs[k + 1], m, te.block_scale(xs[k], m), f"{name} block {k} (broadcast)", slots,
                           *te.BOUNDS["broadcast"])
            xa = None
            continue
        q, q_xs = c3.block(cfg, W, k, xs[k], c3.block_scales(cfg, scales, k), xa=xa)
        f, _ = c3.block(cfg, W, k, xs[k], None, xa=xa)
        d_q, d_qf = float(np.abs(xs[k + 1] - q).mean()), float(np.abs(q - f).mean())
        d_f = float(np.abs(xs[k + 1] - f).mean())
        print(f"{name} batch {batch} block {k}: mean |d| engine to the emulation {d_q:.3e}, emulation to the fp16 "
              f"block {d_qf:.3e} (ratio {d_q / d_qf:.3f}), engine to the fp16 block {d_f:.3e}")
        worst = max(worst, d_q / d_qf)
        assert d_q <= RATIO_BOUND * d_qf, (name, k, d_q, d_qf)
        xa = c3.handed_on(q_xs, xs[k + 1]) if c3.feeds_layerwise(cfg, k) else None
    want = emu.heads(torch.from_numpy(xs[-1]))
    d = np.abs(out["raw"] - np.asarray(want))
    assert d.max() <= te.HEADS_TOL, (name, float(d.max()))
    print(f"{name} batch {batch}: worst ratio {worst:.3f}, heads max |d| {d.max():.2e}")


# ---- 2. whole net ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", c3.NETS)
def test_whole_net_within_three_times_the_emulations_error_to_float64(built, files, name):
    """batch 16 (conv_widths_common.positions()): max |d| of move logits, move probabilities and value probabilities to
    the float64 outputs within int8_conv3_restatement.BOUNDS (three times the emulation's own error)"""
    cfg, W = c3.config(name), c3.weights(name)
    pos = cw.positions()
    ref = cw.outputs(cfg, W, pos, fp16=False)
    eng = _with_scales(files(name), 16)
    got = _run(eng, pos)
    eng.close()
    assert np.isfinite(got["raw"]).all()
    err = c3.errors(got, {k: np.asarray(ref[k]) for k in ("raw", "move_probs", "value_probs")})
    print(f"{name}: {err}")
    for k, bound in c3.BOUNDS[name].items():
        assert err[k] <= bound, (name, k, err)


# ---- 3. both kernel forms; the classic nets' existing plans -----------------------------------------------------------

_FORMS_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from p3achygo_amd import engine, features
d = np.load(sys.argv[1], allow_pickle=True)
cal = np.frombuffer(d["cal"].tobytes(), dtype=features.features_dtype()).copy().reshape(int(d["ncal"]), -1)
pos = features.random_positions(37, seed=43)
out = {}
for key, path, flag in zip(d["keys"], d["paths"], d["flags"]):
    eng = engine.HipEngine(str(path), 37, flags=int(flag))
    for c in cal:
        eng.load_all(c)
        eng.int8_calibrate()
    out[key + ":scales"] = eng.int8_scales()
    eng.load_all(pos)
    eng.RunInference()
    out[key + ":raw"] = np.stack([eng.get_raw(s) for s in range(37)])
    ms, fl, kname = eng.time_trunk_kernel(37, 1)
    out[key + ":kernel"] = np.array(kname)
    eng.close()
np.savez(sys.argv[2], **out)
"""

TEMPLATED = ("test_b3c384btl3", "test_b3c384nbt")
CLASSIC = (("test_b3c192classic", "FLAG_INT8"), ("test_b3c128classic", "FLAG_INT8_ANY"))


@pytest.fixture(scope="module")
def forms(built, files, tmp_path_factory):
    """the two children of test 3, run once: 'own' (no P3HIP_CONV_ANY: the templated nets under the flag; the classic nets
    under the flag and under their existing INT8 flag; the templated nets under FLAG_INT8 for the scales) and 'any'
    (P3HIP_CONV_ANY=1: the templated nets under the flag)"""
    from p3achygo_amd import engine
    tmp = tmp_path_factory.mktemp("forms")
    cal = np.stack(c3.calibration_batches())
    jobs = {"own": [(n + ":conv3", files(n), engine.FLAG_INT8_CONV3) for n in TEMPLATED] +
                   [(n + ":every", files(n), engine.FLAG_INT8) for n in TEMPLATED] +
                   [(n + ":conv3", files(n), engine.FLAG_INT8_CONV3) for n, _ in CLASSIC] +
                   [(n + ":every", files(n), getattr(engine, f)) for n, f in CLASSIC],
            "any": [(n + ":conv3", files(n), engine.FLAG_INT8_CONV3) for n in TEMPLATED]}
    done = {}

    def get(which):
        if which not in done:
            inp, outp = tmp / f"in_{which}.npz", tmp / f"out_{which}.npz"
            np.savez(inp, keys=np.array([j[0] for j in jobs[which]]), paths=np.array([j[1] for j in jobs[which]]),
                     flags=np.array([j[2] for j in jobs[which]]), cal=np.frombuffer(cal.tobytes(), np.uint8),
                     ncal=np.array(len(cal)))
            _child(_FORMS_CHILD, [inp, outp], {"P3HIP_CONV_ANY": "1"} if which == "any" else None)
            done[which] = dict(np.load(outp))
        return done[which]
    return get


@pytest.mark.parametrize("name", TEMPLATED)
def test_templated_shapes_through_both_forms_bit_for_bit(forms, name):
    """P3HIP_CONV_ANY=1: the runtime-width entry points (k_lconv_q8_any, k_lconv_i8_any, k_lconv_i8_f16_any, k_lconv_any)
    on the templated shapes equal the templated ones, raw outputs and scales; the timing hook names the int8 3x3 kernel"""
    own, any_ = forms("own"), forms("any")
    assert str(own[name + ":conv3:kernel"]) == "k_lconv_i8<3,192,192>" and str(any_[name + ":conv3:kernel"]) == "k_lconv_i8_any<3>"
    a, b = own[name + ":conv3:raw"], any_[name + ":conv3:raw"]
    assert np.abs(a).max() > 0 and np.isfinite(a).all()
    assert own[name + ":conv3:scales"].tobytes() == any_[name + ":conv3:scales"].tobytes()
    assert a.tobytes() == b.tobytes(), (name, np.argwhere(a != b)[:5])
    # and the plan is its own: not the results of the engine that quantizes every conv
    assert a.tobytes() != own[name + ":every:raw"].tobytes()


@pytest.mark.parametrize("name,flag", CLASSIC)
def test_classic_nets_equal_their_existing_int8_plan_bit_for_bit(forms, name, flag):
    out = forms("own")
    assert str(out[name + ":conv3:kernel"]) == str(out[name + ":every:kernel"]) and "k_lconv_i8" in str(out[name + ":conv3:kernel"])
    a, b = out[name + ":conv3:raw"], out[name + ":every:raw"]
    assert np.abs(a).max() > 0 and np.isfinite(a).all()
    assert out[name + ":conv3:scales"].tobytes() == out[name + ":every:scales"].tobytes()
    assert a.tobytes() == b.tobytes(), (name, np.argwhere(a != b)[:5])


@pytest.mark.parametrize("name", TEMPLATED)
def test_scales_are_the_3x3_entries_of_the_engine_that_quantizes_every_conv(forms, name):
    """both calibrate through the same fp16 plan: bit for bit the entries of P3HIP_FLAG_INT8's scales at the 3x3 inputs"""
    out = forms("own")
    cfg = c3.config(name)
    every = ar.quantized_tensors(cfg)
    at = [every.index(n) for n in c3.quantized_tensors(cfg)]
    s3, s = out[name + ":conv3:scales"], out[name + ":every:scales"]
    assert len(s) == len(every) and len(s3) == len(at) and (s3 > 0).all()
    assert s3.tobytes() == s[at].tobytes()


# ---- 4. padding is inert ---------------------------------------------------------------------------------------------

def _garbage_twin(cfg, W):
    """(cfg, W) zero-padded to multiples of 64 as the engine pads (conv_widths_common.pad_weights), then garbage wherever
    a padded weight channel cannot reach a real value: the padded output columns of every conv whose output passes a BN
    (all but a block's last conv: the padded channel's folded BN is scale = shift = 0, so its activation is mish(0) = 0
    whatever the conv gave), and the padded input rows of the fp16 1x1 convs (their input there is that exact 0).  The
    padded input rows of a 3x3 conv stay zero: they enter its per-output-channel weight scale."""
    rng = np.random.default_rng(5)
    C, Cb = cfg.channels, cfg.bottleneck_channels
    big, P = cw.pad_weights(cfg, W)
    for i in range(cfg.blocks):
        kind = cfg.block_kind(i)
        if kind == "broadcast":
            continue
        n = ar.n_convs(cfg, kind)
        for j in range(n):
            w = P[f"blocks.{i}.conv{j}.w"]   # [k][k][cin][cout]
            cin, cout = (C if j == 0 else Cb), (C if j == n - 1 else Cb)
            if j < n - 1:
                w[:, :, :cin, cout:] = rng.uniform(-3, 3, w[:, :, :cin, cout:].shape)
            if w.shape[0] == 1:
                w[:, :, cin:, :cout] = rng.uniform(-3, 3, w[:, :, cin:, :cout].shape)
    return big, P


def test_garbage_in_the_padded_weight_channels_changes_no_bit(built, files):
    """test_b3c192btl3 (C_b 96 -> 128 at load) and its padded twin with garbage in the padded channels: bit-identical
    scales and raw outputs.  (The padded twin of test_b3c96nbt is a (128, 64) nbt file, a trunk of the fused block kernel,
    which the flag refuses.)"""
    from p3achygo_amd import features
    pos = features.random_positions(37, seed=43)
    got = []
    for garbage in (False, True):
        eng = _calibrated(files("test_b3c192btl3", garbage=garbage), 37)
        got.append((eng.int8_scales(), _run(eng, pos)["raw"]))
        eng.close()
    assert np.abs(got[0][1]).max() > 0 and (got[0][0] > 0).all()
    assert got[0][0].tobytes() == got[1][0].tobytes()
    assert got[0][1].tobytes() == got[1][1].tobytes()


# ---- 5. calibration --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["test_b3c96nbt", "test_b3c192btl3"])
def test_calibrated_scales_match_the_emulation_and_repeat_bit_for_bit(built, files, name):
    from p3achygo_amd import engine
    cfg, W = c3.config(name), c3.weights(name)
    a = _calibrated(files(name), 16)
    sa = a.int8_scales()
    a.close()
    b = _calibrated(files(name), 16)
    sb = b.int8_scales()
    b.close()
    assert np.array_equal(sa, sb)
    want = c3.minmax_scales(cfg, W, [te.inputs(c) for c in c3.calibration_batches()])
    assert len(sa) == len(want) == len(c3.quantized_tensors(cfg))
    # the engine calibrates on its fp16 plan: equal within a few fp16 roundings of the maxima (tests/test_int8_any_gpu.py)
    np.testing.assert_allclose(sa, want, rtol=4e-3, atol=0)
    # the runtime-width nets: the 3x3 entries of the INT8_ANY engine's scales, bit for bit
    e = _calibrated(files(name), 16, flags=engine.FLAG_INT8_ANY, own=False)
    se = e.int8_scales()
    e.close()
    every = ar.quantized_tensors(cfg)
    assert sa.tobytes() == se[[every.index(n) for n in c3.quantized_tensors(cfg)]].tobytes()


def test_saved_scales_reproduce_the_results_and_bad_calls_fail(built, files):
    from p3achygo_amd import engine, features
    path = files("test_b3c192btl3")
    pos = features.random_positions(24, seed=31)
    a = _calibrated(path, 32)
    want = _run(a, pos)["raw"]
    scales = a.int8_scales()
    a.close()
    b = engine.HipEngine(path, 32, flags=_flag())
    assert len(b.int8_scales()) == len(scales) == 6
    b.LoadBatch(0, pos[:1])
    with pytest.raises(engine.EngineError, match="no activation scales"):
        b.RunInference()
    b.set_int8_scales(scales)
    assert np.array_equal(b.int8_scales(), scales)
    assert np.array_equal(_run(b, pos)["raw"], want)
    with pytest.raises(engine.EngineError, match="quantized tensors"):
        b.set_int8_scales(scales[:-1])
    b.close()


# ---- 6. composition, on one nbt net ----------------------------------------------------------------------------------

def test_compaction_and_run_all_slots_equal_the_plain_engine(built, files):
    from p3achygo_amd import engine, features
    path = files(MECH_NET)
    pos = features.random_positions(20, seed=17)
    plain = _with_scales(path, 20)
    want = _run(plain, pos)["raw"]
    plain.close()
    assert np.abs(want).max() > 0
    slots = list(range(2, 62, 3))              # 20 of 64 slots: compacted to a dense batch of 20
    comp = _with_scales(path, 64)
    assert np.array_equal(_run(comp, pos, slots)["raw"], want)
    comp.close()
    allslots = _with_scales(path, 64, engine.FLAG_RUN_ALL_SLOTS)
    assert np.array_equal(_run(allslots, pos, slots)["raw"], want)
    allslots.close()


def test_launch_graph_replays_bit_for_bit_and_sees_new_scales(built, files):
    from p3achygo_amd import engine, features
    path = files(MECH_NET)
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


def test_repeated_runs_are_bit_identical(built, files):
    from p3achygo_amd import features
    path = files(MECH_NET)
    batch = 128
    pos = np.tile(features.random_positions(32, seed=2, n_games=8), batch // 32).copy()
    seen = set()
    for _ in range(2):
        eng = _with_scales(path, batch)
        for _ in range(3):
            eng.load_all(pos)
            eng.RunInference()
            raw = np.stack([eng.get_raw(s) for s in range(batch)])
            assert np.array_equal(raw[:32], raw[96:])      # copies of a position: bit-identical
            seen.add(raw.tobytes())
        eng.close()
    assert len(seen) == 1


def test_cache_hits_equal_the_evaluation(built, files):
    from p3achygo_amd import features
    path = files(MECH_NET)
    pos = features.random_positions(16, seed=12)
    ref = _with_scales(path, 16)
    want = _run(ref, pos)["raw"]
    ref.close()
    eng = _with_scales(path, 16)
    eng.EnableCache(8)
    for rnd in range(2):
        for i in range(16):
            eng.LoadBatchKeyed(i, pos[i:i + 1], 1000 + i, 77)
        eng.RunInference()
        for i in range(16):
            if rnd == 0:
                assert np.array_equal(eng.get_raw(i), want[i])
            r, _, hit = eng.GetBatchKeyed(i)
            assert hit == (rnd == 1)
            assert np.array_equal(np.ctypeslib.as_array(r.move_logits), want[i][:362].astype(np.float32))
    eng.close()


def test_trunk_kernel_timing_names_the_int8_3x3_kernel(built, files):
    from p3achygo_amd import features
    for name, kernel in ((MECH_NET, "k_lconv_i8_any<3>"), ("test_b3c384btl3", "k_lconv_i8<3,192,192>")):
        cfg = c3.config(name)
        eng = _with_scales(files(name), 16)
        eng.load_all(features.random_positions(16, seed=3))
        eng.upload()
        ms, flops, kname = eng.time_trunk_kernel(16, 2)
        eng.close()
        assert kname == kernel and ms > 0
        w3 = cfg.bottleneck_channels                      # the file's own width, not the padded one
        assert flops == 2.0 * 9 * w3 * w3 * 361 * 16


def test_aux_on_top_keeps_every_other_outputs_bits(built, files):
    from p3achygo_amd import engine, features
    path = files(MECH_NET)
    pos = features.random_positions(16, seed=5)
    plain = _with_scales(path, 16)
    want = _run(plain, pos)
    plain.close()
    aux = _with_scales(path, 16, engine.FLAG_AUX)
    got = _run(aux, pos)
    recs = np.stack([aux.GetAux(s) for s in range(16)])
    aux.close()
    for k in want:
        assert want[k].tobytes() == got[k].tobytes(), k
    assert np.isfinite(recs).all() and np.abs(recs).max() > 0
