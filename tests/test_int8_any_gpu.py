"""Calibrated INT8 at any width on the MI355X (P3HIP_FLAG_INT8_ANY, DESIGN.md section 9 "INT8 at any width").

Every engine here is calibrated on tests/int8_restatement.calibration_batches() (or loads the scales of one that was).
The nets (int8_any_restatement.NETS) are three or four blocks, chosen for where k_lconv_i8_any can break: one slice per
conv, padded widths, odd slice counts, the nbt dual / res flows, the classic 3x3 from the raw stream, five slices, and
broadcast blocks between layer-wise blocks at the wide end.

Accuracy: block by block, teacher-forced, against the CPU emulation of the same scheme run from the engine's own x and
with the engine's own scales (mean |d| to the INT8 emulation below RATIO_BOUND of the mean |d| between that emulation and
the unquantized fp16 block: the engine implements the scheme, it is not merely close to fp16), and the whole net
against the float64 outputs within int8_any_restatement.BOUNDS.  Everything else is bit for bit: the templated shapes
through both forms of the kernel, the other INT8 flags' plans, an explicitly padded twin, saved scales, compaction,
RUN_ALL_SLOTS, graph replay, repeats, AUX.

Measured on one MI355X (test_blocks_teacher_forced, the ratio per layer-wise block, bound 0.5): 0.000 - 0.014 on every
net, batch and block but the first block of test_b3c320nbt at batch 1, 0.129; heads max |d| 2.3e-6.  Whole nets, largest
move-logit error to float64: 0.009 (test_b3c64btl2) to 0.053 (test_b3c128nbt), 0.25 - 0.34 of the bounds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_widths_common as cw  # noqa: E402
import int8_any_restatement as ar  # noqa: E402
import int8_gpu_common as gc  # noqa: E402
import trunk_emulation as te  # noqa: E402

pytestmark = pytest.mark.gpu

RATIO_BOUND = 0.5          # tests/test_int8_block_gpu.py
BLOCK_BATCHES = (1, 37)
FUSED_FP16 = ("test_b3c128nbt", "test_b3c256nbt")   # their fp16 plan is the fused block kernel's, not conv_any.hip's
MECH_NET = "test_b3c128nbt"
CHILD_TIMEOUT = 240


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> .p3w of netspec.generate_weights(cfg, randomize=True); padded=True: its explicitly zero-padded twin"""
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("int8_any")
    cache = {}

    def get(name, padded=False):
        key = (name, padded)
        if key not in cache:
            cfg, W = ar.config(name), ar.weights(name)
            if padded:
                cfg, W = cw.pad_weights(cfg, W)
            cache[key] = os.path.join(d, name + ("_padded" if padded else "") + ".p3w")
            netspec.save_p3w(cache[key], cfg, W)
        return cache[key]
    return get


_E = gc.Engines("FLAG_INT8_ANY", raw_f64=False)
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
eng = engine.HipEngine(path, 16, flags=engine.FLAG_INT8_ANY)
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
    eng = engine.HipEngine(path, len(pos), flags=engine.FLAG_INT8_ANY)
    eng.set_int8_scales(scales)
    eng.load_all(pos)
    eng.RunInference()
    out["x%%d" %% stop] = eng.debug_x(len(pos), Cp)[slots]
    out["a%%d" %% stop] = eng.debug_act_i8(len(pos), Cp)[slots]
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


@pytest.mark.parametrize("batch", BLOCK_BATCHES)
@pytest.mark.parametrize("name", ar.NETS)
def test_blocks_teacher_forced(built, files, tmp_path, name, batch):
    """The engine's x after block k against the emulation of block k from the engine's x after block k - 1 (and, where
    block k - 1 is layer-wise too, the engine's own int8 input of the block's first conv, p3hip_debug_act_i8: the engine
    quantized it from an fp32 sum it does not store; the fp16 yardstick takes int8_any_restatement.handed_on's estimate
    of that sum) with the engine's scales: mean |d| to the INT8 emulation below 0.5 of the mean |d| between that emulation and the unquantized
    fp16 block.  The stem, the broadcast blocks and the heads (the fp16 engine's kernels) by trunk_emulation's bounds, and
    the stem bit for bit the fp16 engine's where that runs the same plan (conv_any.hip; the fp16 engine of the (128, 64)
    and (256, 128) nbt nets is the fused block kernel's plan with the templated stem, another kernel: one fp16 ulp apart
    in places); padded channels of the stream are exactly 0."""
    import torch
    from test_conv_widths_gpu import block_batch
    cfg, W = ar.config(name), ar.weights(name)
    C, Cp = cfg.channels, cw.padded(cfg.channels)
    pos, slots = block_batch(batch)
    cal = np.stack(ar.calibration_batches())
    inp, outp = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(inp, path=np.array(files(name)), Cp=np.array(Cp), blocks=np.array(cfg.blocks), slots=slots,
             pos=np.frombuffer(pos.tobytes(), np.uint8), cal=np.frombuffer(cal.tobytes(), np.uint8), ncal=np.array(len(cal)))
    _child(_BLOCKS_CHILD, [inp, outp])
    out = np.load(outp)
    scales = out["scales"]
    assert len(scales) == len(ar.quantized_tensors(cfg)) and (scales > 0).all()
    full = [out[f"x{s}"] for s in range(cfg.blocks + 1)]
    assert np.abs(full[0]).max() > 0
    if name not in FUSED_FP16:
        assert out["x0_fp16"].tobytes() == full[0].tobytes()
    for x in full:
        assert np.isfinite(x).all() and np.all(x[:, C:] == 0)
    xs = [x[:, :C].astype(np.float64).reshape(len(slots), C, 19, 19) for x in full]
    emu = cw.trunk(cfg, W)
    x0 = emu.stem(pos[slots])
    te.check_block(xs[0], x0, te.rms(x0), f"{name} stem", slots, *te.BOUNDS["stem"])
    xa_f = None   # the fp16 yardstick's estimate of the sum handed on
    worst = 0.0
    for k in range(cfg.blocks):
        if cfg.block_kind(k) == "broadcast":
            m = emu.block(k, torch.from_numpy(xs[k]))
            te.check_block(xs[k + 1], m, te.block_scale(xs[k], m), f"{name} block {k} (broadcast)", slots,
                           *te.BOUNDS["broadcast"])
            xa_f = None
            continue
        # what the block's first conv read: after another layer-wise block the engine's own int8 tensor (its codes
        # were taken from an fp32 sum that is not stored); after the stem or a broadcast block mish(bn0(x)) of the stored x
        codes = out[f"a{k}"][:, :C] if k > 0 and ar.feeds_layerwise(cfg, k - 1) else None
        if codes is not None:
            assert np.all(out[f"a{k}"][:, C:] == 0) and np.abs(codes).max() > 0
        q, q_xs = ar.block(cfg, W, k, xs[k], ar.block_scales(cfg, scales, k), codes=codes)
        f, f_xs = ar.block(cfg, W, k, xs[k], None, xa=xa_f)
        d_q, d_qf = float(np.abs(xs[k + 1] - q).mean()), float(np.abs(q - f).mean())
        d_f = float(np.abs(xs[k + 1] - f).mean())
        print(f"{name} batch {batch} block {k}: mean |d| engine to the INT8 emulation {d_q:.3e}, emulation to the fp16 "
              f"block {d_qf:.3e} (ratio {d_q / d_qf:.3f}), engine to the fp16 block {d_f:.3e}")
        worst = max(worst, d_q / d_qf)
        assert d_q < RATIO_BOUND * d_qf, (name, k, d_q, d_qf)
        xa_f = ar.handed_on(f_xs, xs[k + 1]) if ar.feeds_layerwise(cfg, k) else None
    want = emu.heads(torch.from_numpy(xs[-1]))
    d = np.abs(out["raw"] - np.asarray(want))
    assert d.max() <= te.HEADS_TOL, (name, float(d.max()))
    print(f"{name} batch {batch}: worst ratio {worst:.3f}, heads max |d| {d.max():.2e}")


# ---- 2. whole net ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ar.NETS)
def test_whole_net_within_the_emulation_bounds_of_float64(built, files, name):
    """batch 16 (conv_widths_common.positions()): max |d| of move logits, move probabilities and value probabilities to
    the float64 outputs within int8_any_restatement.BOUNDS (three times the emulation's own error)"""
    cfg, W = ar.config(name), ar.weights(name)
    pos = cw.positions()
    ref = cw.outputs(cfg, W, pos, fp16=False)
    eng = _with_scales(files(name), 16)
    got = _run(eng, pos)
    eng.close()
    assert np.isfinite(got["raw"]).all()
    err = ar.errors(got, {k: np.asarray(ref[k]) for k in ("raw", "move_probs", "value_probs")})
    print(f"{name}: {err}")
    for k, bound in ar.BOUNDS[name].items():
        assert err[k] <= bound, (name, k, err)


# ---- 3. same kernels, both forms; the other flags' plans -------------------------------------------------------------

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

TEMPLATED = ("test_b3c384btl3", "test_b3c384nbt", "test_b3c192classic")
FUSED = (("test_b3c256btl1", "FLAG_INT8_FUSED"), ("test_b3c128btl2", "FLAG_INT8_C128"))


@pytest.fixture(scope="module")
def forms(built, weight_files, tmp_path_factory):
    """the two children of test 3, run once: 'own' (no P3HIP_CONV_ANY: every net under the flag that serves it, the two
    fused ones under FLAG_INT8_ANY too) and 'any' (P3HIP_CONV_ANY=1: the templated nets under FLAG_INT8_ANY)"""
    from p3achygo_amd import engine
    tmp = tmp_path_factory.mktemp("forms")
    cal = np.stack(ar.calibration_batches())
    jobs = {"own": [(n + ":own", weight_files(n), engine.FLAG_INT8) for n in TEMPLATED] +
                   [(n + ":own", weight_files(n), getattr(engine, f)) for n, f in FUSED] +
                   [(n + ":any", weight_files(n), engine.FLAG_INT8_ANY) for n, _ in FUSED],
            "any": [(n + ":any", weight_files(n), engine.FLAG_INT8_ANY) for n in TEMPLATED]}
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
    """P3HIP_CONV_ANY=1 and FLAG_INT8_ANY: k_lconv_i8_any on the ten templated shapes equals k_lconv_i8 under FLAG_INT8,
    raw outputs and scales"""
    own, any_ = forms("own"), forms("any")
    assert str(own[name + ":own:kernel"]) == "k_lconv_i8<3,192,192>" and str(any_[name + ":any:kernel"]) == "k_lconv_i8_any<3>"
    a, b = own[name + ":own:raw"], any_[name + ":any:raw"]
    assert np.abs(a).max() > 0 and np.isfinite(a).all()
    assert own[name + ":own:scales"].tobytes() == any_[name + ":any:scales"].tobytes()
    assert a.tobytes() == b.tobytes(), (name, np.argwhere(a != b)[:5])


@pytest.mark.parametrize("name,flag", FUSED)
def test_fused_shapes_take_their_own_flags_plan_bit_for_bit(forms, name, flag):
    out = forms("own")
    assert str(out[name + ":any:kernel"]) == str(out[name + ":own:kernel"]) and "k_block_i8" in str(out[name + ":any:kernel"])
    a, b = out[name + ":own:raw"], out[name + ":any:raw"]
    assert np.abs(a).max() > 0 and np.isfinite(a).all()
    assert out[name + ":own:scales"].tobytes() == out[name + ":any:scales"].tobytes()
    assert a.tobytes() == b.tobytes(), (name, np.argwhere(a != b)[:5])


# ---- 4. padding is inert ---------------------------------------------------------------------------------------------

def test_padding_is_inert(built, files):
    """test_b3c96nbt (C 96 -> 128, C_b 48 -> 64 at load) and its twin whose file holds the zero padding: bit-identical
    scales and raw outputs"""
    from p3achygo_amd import features
    pos = features.random_positions(37, seed=43)
    got = []
    for padded in (False, True):
        eng = _calibrated(files("test_b3c96nbt", padded=padded), 37)
        got.append((eng.int8_scales(), _run(eng, pos)["raw"]))
        eng.close()
    assert np.abs(got[0][1]).max() > 0 and (got[0][0] > 0).all()
    assert got[0][0].tobytes() == got[1][0].tobytes()
    assert got[0][1].tobytes() == got[1][1].tobytes()


# ---- 5. calibration --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["test_b3c96nbt", "test_b3c192btl3", "test_b3c128classic"])
def test_calibrated_scales_match_the_emulation_and_repeat_bit_for_bit(built, files, name):
    cfg, W = ar.config(name), ar.weights(name)
    a = _calibrated(files(name), 16)
    sa = a.int8_scales()
    a.close()
    b = _calibrated(files(name), 16)
    sb = b.int8_scales()
    b.close()
    assert np.array_equal(sa, sb)
    want = ar.minmax_scales(cfg, W, [te.inputs(c) for c in ar.calibration_batches()])
    assert len(sa) == len(want) == len(ar.quantized_tensors(cfg))
    # the engine calibrates on its fp16 plan: equal within a few fp16 roundings of the maxima
    np.testing.assert_allclose(sa, want, rtol=4e-3, atol=0)


def test_saved_scales_reproduce_the_results_and_bad_calls_fail(built, files):
    from p3achygo_amd import engine, features
    path = files("test_b3c320nbt")
    pos = features.random_positions(24, seed=31)
    a = _calibrated(path, 32)
    want = _run(a, pos)["raw"]
    scales = a.int8_scales()
    a.close()
    b = engine.HipEngine(path, 32, flags=_flag())
    assert len(b.int8_scales()) == len(scales) == 12
    b.LoadBatch(0, pos[:1])
    with pytest.raises(engine.EngineError, match="no activation scales"):
        b.RunInference()
    b.set_int8_scales(scales)
    assert np.array_equal(b.int8_scales(), scales)
    assert np.array_equal(_run(b, pos)["raw"], want)
    with pytest.raises(engine.EngineError, match="quantized tensors"):
        b.set_int8_scales(scales[:-1])
    b.close()


# ---- 6. engine mechanics, on one nbt net -----------------------------------------------------------------------------

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


def test_trunk_kernel_timing_names_the_runtime_width_kernel(built, files):
    from p3achygo_amd import features
    for name in (MECH_NET, "test_b3c96nbt"):
        cfg = ar.config(name)
        eng = _with_scales(files(name), 16)
        eng.load_all(features.random_positions(16, seed=3))
        eng.upload()
        ms, flops, kname = eng.time_trunk_kernel(16, 2)
        eng.close()
        assert kname == "k_lconv_i8_any<3>" and ms > 0
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
