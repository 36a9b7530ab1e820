"""Calibrated INT8 at any width (P3HIP_FLAG_INT8_ANY), without a GPU: the emulation's own error against the float64
outputs (tests/int8_any_restatement.py), the quantized tensors of every block kind, what p3hip_create answers for the
flag (through engine.HipEngine, as tests/test_create_matrix_cpu.py asks, and through the host-side plan hook
p3hip_debug_plan, which names the path chosen), the padded weights' quantization, and the compiled resources of the
runtime-width kernels (csrc/lconv_i8_any.hip)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_widths_common as cw  # noqa: E402
import int8_any_restatement as ar  # noqa: E402
import trunk_emulation as te  # noqa: E402
from test_create_matrix_cpu import outcome  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> .p3w of netspec.generate_weights(cfg, randomize=True); (name, "padded"): its explicitly zero-padded twin"""
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


@pytest.mark.parametrize("name", ar.NETS)
def test_emulation_error_is_within_half_the_gpu_bounds(name):
    err, scales = ar.emulation_errors(name)
    assert len(scales) == len(ar.quantized_tensors(ar.config(name))) and (scales > 0).all()
    print(name, err)
    for k, bound in ar.BOUNDS[name].items():
        assert err[k] <= 0.5 * bound, (name, k, err)
        # the table in the file is what was measured, and the bound is made from it by the stated rule
        m = max(v[("logit", "prob", "value_prob").index(k)] for v in ar.MEASURED[name])
        assert 3 * m <= bound <= 3 * m * 1.2, (name, k, m, bound)


def test_emulation_equals_the_layerwise_one_on_a_templated_shape():
    """one scheme: on test_b3c192classic the forward pass here is int8_restatement.forward, bit for bit"""
    import int8_restatement as ir
    from p3achygo_amd import netspec
    cfg = netspec.CONFIGS["test_b3c192classic"]
    W = netspec.generate_weights(cfg, randomize=True)
    planes, sc = te.inputs(cw.positions(3))
    s = ir.minmax_scales(cfg, W, [(planes, sc)])
    assert np.array_equal(s, ar.minmax_scales(cfg, W, [(planes, sc)]))
    a, b = ir.forward(cfg, W, planes, sc, scales=s), ar.forward(cfg, W, planes, sc, scales=s)
    assert np.array_equal(np.asarray(a["raw"]), np.asarray(b["raw"]))


@pytest.mark.parametrize("name,per_block,blocks", [
    ("test_b3c64btl2", 4, 2), ("test_b3c192btl3", 5, 2), ("test_b3c96nbt", 6, 2), ("test_b3c256nbt", 6, 2),
    ("test_b3c128classic", 2, 2), ("test_b4c512btl3_i2", 5, 2)])
def test_quantized_tensors_of_every_block_kind(files, name, per_block, blocks):
    """btl (inner + 2), nbt (6), classic (2); broadcast blocks (the last block of each net; test_b4c512btl3_i2: blocks 1
    and 3) have none; the engine's plan counts the same"""
    from p3achygo_amd import engine
    cfg = ar.config(name)
    names = ar.quantized_tensors(cfg)
    assert sum(cfg.block_kind(i) != "broadcast" for i in range(cfg.blocks)) == blocks
    assert len(names) == per_block * blocks
    assert not any(cfg.block_kind(int(n.split(".")[1])) == "broadcast" for n in names)
    assert [len(ar.block_scales(cfg, np.arange(len(names)), k)) for k in range(cfg.blocks)
            if cfg.block_kind(k) != "broadcast"] == [per_block] * blocks
    path, n_q, digest = engine.debug_plan(files(name), engine.FLAG_INT8_ANY)
    assert (path, n_q) == ("Int8Any", len(names)) and digest != 0
    # the emulation's calibration visits them in that order, one maximum each
    obs = []
    planes, sc = te.inputs(cw.positions(1))
    ar.forward(cfg, ar.weights(name), planes, sc, observe=obs)
    assert len(obs) == len(names) and all(v > 0 for v in obs)


@pytest.mark.parametrize("name", ar.NETS)
def test_the_flag_is_accepted_on_every_test_net(built, files, name):
    from p3achygo_amd import engine
    assert outcome(files(name), engine.FLAG_INT8_ANY) == "accepted"
    assert engine.debug_plan(files(name), engine.FLAG_INT8_ANY)[0] == "Int8Any"
    # and without it nothing changed: the fp16 plan of the net
    want = "Fused" if name in ("test_b3c128nbt", "test_b3c256nbt") else "ConvAny"
    assert engine.debug_plan(files(name), 0)[0] == want
    for other in (engine.FLAG_INT8, engine.FLAG_INT8_FUSED, engine.FLAG_INT8_C128):
        assert outcome(files(name), other) != "accepted"


def test_refusals_have_messages_of_their_own(built, files, tmp_path):
    from p3achygo_amd import engine, netspec
    F = engine.FLAG_INT8_ANY
    tfm = str(tmp_path / "tfm.p3w")
    cfg = netspec.get_config("test_b2d64h2_tfm")
    netspec.save_p3w(tfm, cfg, netspec.generate_weights(cfg, randomize=True))
    for flags in (F, F | engine.FLAG_INT8, F | engine.FLAG_FP32_TFM):     # the transformer's message comes first
        with pytest.raises(engine.EngineError, match="transformer.*have no INT8 plan") as ex:
            engine.HipEngine(tfm, 4, flags=flags)
        assert netspec.TRANSFORMER_SET in str(ex.value) and "P3HIP_FLAG_INT8_ANY" in str(ex.value)
    conv = files("test_b3c96nbt")
    for other in (engine.FLAG_INT8, engine.FLAG_INT8_FUSED, engine.FLAG_INT8_C128):
        with pytest.raises(engine.EngineError, match="P3HIP_FLAG_INT8_ANY cannot be combined with P3HIP_FLAG_INT8, "):
            engine.HipEngine(conv, 4, flags=F | other)
    for other in (engine.FLAG_FP32, engine.FLAG_FP32_TFM, engine.FLAG_FP32_ANY):
        with pytest.raises(engine.EngineError, match="P3HIP_FLAG_INT8_ANY cannot be combined with P3HIP_FLAG_FP32.*an "
                                                     "engine runs one precision plan"):
            engine.HipEngine(conv, 4, flags=F | other)
    # a conv trunk outside P3HIP_CONV_SET stays what it was
    assert outcome_of("tiny", F, tmp_path).startswith("unsupported architecture")


def outcome_of(name, flags, directory):
    from p3achygo_amd import netspec
    cfg = netspec.get_config(name)
    path = os.path.join(str(directory), name + ".p3w")
    netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
    return outcome(path, flags)


@pytest.mark.parametrize("name,own,path", [
    ("test_b3c384btl3", "INT8", "Int8"), ("test_b3c384nbt", "INT8", "Int8"), ("test_b3c192classic", "INT8", "Int8"),
    ("test_b3c256btl1", "INT8_FUSED", "Int8Fused256"), ("test_b5c256btl2_i2", "INT8_FUSED", "Int8Fused256"),
    ("test_b3c128btl2", "INT8_C128", "Int8Fused128")])
def test_fused_and_templated_shapes_resolve_to_their_existing_plans(built, weight_files, monkeypatch, name, own, path):
    """the path, the tensor count and the quantized weights of the flag that serves the shape on its own"""
    from p3achygo_amd import engine
    monkeypatch.delenv("P3HIP_CONV_ANY", raising=False)
    f = weight_files(name)
    got = engine.debug_plan(f, engine.FLAG_INT8_ANY)
    assert got[0] == path and got == engine.debug_plan(f, getattr(engine, "FLAG_" + own))
    assert outcome(f, engine.FLAG_INT8_ANY) == "accepted"
    # P3HIP_CONV_ANY=1 sends the templated layer-wise shapes, and only those, to the runtime-width kernels: the same
    # quantized weights in the same order; and P3HIP_FLAG_INT8 itself stays as it is
    monkeypatch.setenv("P3HIP_CONV_ANY", "1")
    sw = engine.debug_plan(f, engine.FLAG_INT8_ANY)
    assert sw == (("Int8Any",) + got[1:] if own == "INT8" else got)
    assert engine.debug_plan(f, getattr(engine, "FLAG_" + own)) == got


def test_padded_weights_quantize_as_the_explicitly_padded_twin(built, files):
    """test_b3c96nbt (C 96 -> 128, C_b 48 -> 64) and its twin whose file already holds the zero padding: the same int8
    weight bytes and weight scales (pack_lconv_i8 runs on the padded weights: a padded output channel has scale 0 and
    q = 0, a padded input channel q = 0), the same tensor count"""
    from p3achygo_amd import engine
    a = engine.debug_plan(files("test_b3c96nbt"), engine.FLAG_INT8_ANY)
    b = engine.debug_plan(files("test_b3c96nbt", padded=True), engine.FLAG_INT8_ANY)
    assert a == b and a[0] == "Int8Any" and a[1] == 12 and a[2] != 0
    # the digest tells weights apart: another net of the same shape family has another
    assert engine.debug_plan(files("test_b3c128nbt"), engine.FLAG_INT8_ANY)[2] != a[2]


def test_runtime_width_kernels_keep_two_workgroups_per_cu_and_no_scratch():
    """the ten flag sets of k_lconv_i8_any: no scratch, at most 256 VGPRs (two 256-thread workgroups per CU), the int8
    MFMA, and the LDS image of two 28,224-byte slices whatever the widths"""
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "lconv_i8_any.hip"), "-o", "-"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = r.stdout
    seen = 0
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S*k_lconv_i8_any\S*)\s*$", asm, re.M):
        name = m.group(1)
        desc = asm[m.start():asm.index(".end_amdhsa_kernel", m.start())]
        vg = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", desc).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1))
        start = re.search(r"^" + re.escape(name) + r":", asm, re.M).start()
        body = asm[start:asm.index(".Lfunc_end", start)]
        assert scratch == 0 and "scratch_" not in body, name
        assert vg <= 256, (name, vg)
        assert body.count("v_mfma_i32_16x16x64_i8") > 0, name
        seen += 1
    assert seen == 10
