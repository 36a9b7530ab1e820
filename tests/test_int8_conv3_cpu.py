"""Calibrated INT8 for the 3x3 convs only (P3HIP_FLAG_INT8_CONV3), without a GPU: the plan p3hip_create would build
(p3hip_debug_plan: the path and the quantized tensors, the 3x3 inputs alone), every refusal by a piece of its text, the
emulation's own error against the float64 outputs (tests/int8_conv3_restatement.py), and the compiled resources of the two
new epilogue forms (csrc/lconv_conv3.hip)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_widths_common as cw  # noqa: E402
import int8_any_restatement as ar  # noqa: E402
import int8_conv3_restatement as c3  # noqa: E402
import trunk_emulation as te  # noqa: E402
from test_create_matrix_cpu import outcome  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> .p3w of netspec.generate_weights(cfg, randomize=True)"""
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("int8_conv3")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = os.path.join(d, name + ".p3w")
            netspec.save_p3w(cache[name], c3.config(name), c3.weights(name))
        return cache[name]
    return get


def _flag():
    from p3achygo_amd import engine
    return engine.FLAG_INT8_CONV3


# ---- the plan ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,per_block", [("test_b3c384btl3", 3), ("test_b3c384nbt", 4), ("test_b3c192btl3", 3),
                                            ("test_b3c96nbt", 4), ("test_b3c64btl2", 2)])
def test_plan_is_int8conv3_with_the_3x3_inputs_quantized(built, files, monkeypatch, name, per_block):
    """a btl, an nbt and padded-width nets: n_q = the 3x3 convs (the inner layers per btl block, 4 per nbt block), in the
    emulation's order; P3HIP_CONV_ANY=1 keeps the path, the count and the int8 weights"""
    from p3achygo_amd import engine
    monkeypatch.delenv("P3HIP_CONV_ANY", raising=False)
    cfg = c3.config(name)
    names = c3.quantized_tensors(cfg)
    blocks = sum(cfg.block_kind(i) != "broadcast" for i in range(cfg.blocks))
    assert len(names) == per_block * blocks
    got = engine.debug_plan(files(name), _flag())
    assert got[:2] == ("Int8Conv3", len(names)) and got[2] != 0
    assert outcome(files(name), _flag()) == "accepted"
    # fewer tensors than the plan that quantizes every conv, and other weights in the digest
    every = engine.debug_plan(files(name), engine.FLAG_INT8_ANY)
    assert every[1] == len(ar.quantized_tensors(cfg)) > got[1] and every[2] != got[2]
    # without the flag nothing changed
    assert engine.debug_plan(files(name), 0)[0] == ("Layerwise" if "c384" in name else "ConvAny")
    monkeypatch.setenv("P3HIP_CONV_ANY", "1")
    assert engine.debug_plan(files(name), _flag()) == got
    # the emulation's calibration visits the same tensors, one maximum each
    obs = []
    planes, sc = te.inputs(cw.positions(1))
    c3.forward(cfg, c3.weights(name), planes, sc, observe=obs)
    assert len(obs) == len(names) and all(v > 0 for v in obs)


@pytest.mark.parametrize("name,own", [("test_b3c192classic", "FLAG_INT8"), ("test_b3c128classic", "FLAG_INT8_ANY")])
def test_classic_nets_take_the_existing_int8_plan(built, files, monkeypatch, name, own):
    """only 3x3 convs: the path, n_q (2 per block) and the digest of the net's existing INT8 plan"""
    from p3achygo_amd import engine
    monkeypatch.delenv("P3HIP_CONV_ANY", raising=False)
    got = engine.debug_plan(files(name), _flag())
    assert got == engine.debug_plan(files(name), getattr(engine, own))
    cfg = c3.config(name)
    assert got[1] == len(c3.quantized_tensors(cfg)) == len(ar.quantized_tensors(cfg)) and got[2] != 0
    assert outcome(files(name), _flag()) == "accepted"
    monkeypatch.setenv("P3HIP_CONV_ANY", "1")
    assert engine.debug_plan(files(name), _flag()) == engine.debug_plan(files(name), engine.FLAG_INT8_ANY)


def test_emulation_of_a_classic_net_is_the_existing_one_bit_for_bit():
    import int8_restatement as ir
    cfg, W = c3.config("test_b3c192classic"), c3.weights("test_b3c192classic")
    planes, sc = te.inputs(cw.positions(3))
    s = ir.minmax_scales(cfg, W, [(planes, sc)])
    assert np.array_equal(s, c3.minmax_scales(cfg, W, [(planes, sc)]))
    a, b = ir.forward(cfg, W, planes, sc, scales=s), c3.forward(cfg, W, planes, sc, scales=s)
    assert np.array_equal(np.asarray(a["raw"]), np.asarray(b["raw"]))


# ---- refusals ---------------------------------------------------------------------------------------------------------

def _save(name, directory):
    from p3achygo_amd import netspec
    cfg = netspec.get_config(name)
    path = os.path.join(str(directory), name + ".p3w")
    netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
    return path


def test_every_refusal_names_the_flag(built, files, tmp_path):
    from p3achygo_amd import engine, netspec
    F = _flag()

    def refused(path, flags, match):
        with pytest.raises(engine.EngineError, match=match) as ex:
            engine.HipEngine(path, 4, flags=flags)
        assert "P3HIP_FLAG_INT8_CONV3" in str(ex.value)
        with pytest.raises(engine.EngineError, match=match):
            engine.debug_plan(path, flags)

    tfm = _save("test_b2d64h2_tfm", tmp_path)
    for flags in (F, F | engine.FLAG_INT8, F | engine.FLAG_FP32_TFM, F | engine.FLAG_LOW_LATENCY_TFM):
        refused(tfm, flags, "transformer.*have no INT8 plan")   # the transformer's message comes first
    # the trunks of the fused block kernel, btl and nbt at both widths
    for name in ("test_b3c256btl1", "test_b3c128btl2", "test_b3c128nbt", "test_b3c256nbt"):
        refused(_save(name, tmp_path), F, "fused block kernel.*P3HIP_FLAG_INT8_FUSED, P3HIP_FLAG_INT8_C128 and P3HIP_FLAG_INT8_ANY")
    for conv in (files("test_b3c384btl3"), files("test_b3c96nbt"), files("test_b3c192classic")):
        for other in (engine.FLAG_INT8, engine.FLAG_INT8_FUSED, engine.FLAG_INT8_C128, engine.FLAG_INT8_ANY):
            refused(conv, F | other, "P3HIP_FLAG_INT8_CONV3 cannot be combined with P3HIP_FLAG_INT8, .*one INT8 plan")
        for other in (engine.FLAG_FP32, engine.FLAG_FP32_TFM, engine.FLAG_FP32_ANY):
            refused(conv, F | other, "P3HIP_FLAG_INT8_CONV3 cannot be combined with P3HIP_FLAG_FP32 .*one precision plan")
        for other in (engine.FLAG_LOW_LATENCY, engine.FLAG_LOW_LATENCY_TFM):
            refused(conv, F | other, "P3HIP_FLAG_INT8_CONV3 cannot be combined with P3HIP_FLAG_LOW_LATENCY ")
    # a conv trunk outside P3HIP_CONV_SET stays what it was
    assert outcome(_save("tiny", tmp_path), F).startswith("unsupported architecture")


def test_the_flag_composes_on_the_host_side(built, files):
    """the flags that stand beside P3HIP_FLAG_INT8 leave the plan alone"""
    from p3achygo_amd import engine
    f = files("test_b3c96nbt")
    want = engine.debug_plan(f, _flag())
    for extra in (engine.FLAG_RUN_ALL_SLOTS, engine.FLAG_SHARED_DEVICE, engine.FLAG_LAUNCH_GRAPH, engine.FLAG_AUX,
                  engine.FLAG_SYMMETRY_AVG, engine.FLAG_SYMMETRY_SLOT):
        assert engine.debug_plan(f, _flag() | extra) == want


# ---- the emulation's error: the bounds of the GPU tests ---------------------------------------------------------------

@pytest.mark.parametrize("name", c3.NETS)
def test_emulation_error_is_recorded_as_the_nets_bound(name):
    """the move-logit, move-probability and value-probability error of the emulation against float64 is what
    int8_conv3_restatement.MEASURED records (within the spread of two measurements), BOUNDS is three times the larger
    measurement rounded up, and the emulation stays within half of it"""
    err, scales = c3.emulation_errors(name)
    assert len(scales) == len(c3.quantized_tensors(c3.config(name))) and (scales > 0).all()
    print(name, err, "INT8 with every conv quantized:", c3.INT8_ALL_CONVS[name])
    for i, k in enumerate(("logit", "prob", "value_prob")):
        bound = c3.BOUNDS[name][k]
        m = max(v[i] for v in c3.MEASURED[name])
        assert err[k] <= 0.5 * bound, (name, k, err)
        assert 3 * m <= bound <= 3 * m * 1.2, (name, k, m, bound)
        assert abs(err[k] - c3.MEASURED[name][0][i]) <= 0.01 * c3.MEASURED[name][0][i], (name, k, err)


# ---- kernel resources -------------------------------------------------------------------------------------------------

def test_new_instantiations_use_no_scratch_and_fit_their_launch():
    """csrc/lconv_conv3.hip: eight entry points over k_lconv's body (fp16 1x1, quantized output: pre or not, act or dual,
    templated and runtime-width) and four over k_lconv_i8's (int8 3x3, fp16 output: act, res + dual).  From the code
    object's metadata: no scratch, no spill, at most 256 VGPRs (two 256-thread workgroups per CU), no static LDS (the
    launchers request all of it dynamically: the fp16 form's act buffer + ring, two int8 slice images), and the MFMA of
    each body."""
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "lconv_conv3.hip"), "-o", "-"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = r.stdout
    seen = {"k_lconv_q8": 0, "k_lconv_q8_any": 0, "k_lconv_i8_f16": 0, "k_lconv_i8_f16_any": 0}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\s*$", asm, re.M):
        name = m.group(1)
        kind = re.search(r"\d+(k_lconv_(?:q8|i8_f16)(?:_any)?)I", name).group(1)
        desc = asm[m.start():asm.index(".end_amdhsa_kernel", m.start())]
        vg = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", desc).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1))
        start = re.search(r"^" + re.escape(name) + r":", asm, re.M).start()
        body = asm[start:asm.index(".Lfunc_end", start)]
        assert scratch == 0 and "scratch_" not in body, name
        assert vg <= 256 and lds == 0, (name, vg, lds)
        mfma = "v_mfma_i32_16x16x64_i8" if "i8_f16" in kind else "v_mfma_f32_32x32x16_f16"
        assert body.count(mfma) > 0, name
        seen[kind] += 1
    assert seen == {"k_lconv_q8": 4, "k_lconv_q8_any": 4, "k_lconv_i8_f16": 2, "k_lconv_i8_f16_any": 2}
    for spill in re.findall(r"\.(?:vgpr|sgpr)_spill_count:\s+(\d+)", asm):
        assert int(spill) == 0
