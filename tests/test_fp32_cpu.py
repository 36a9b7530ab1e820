"""The fp32 plan of the conv trunks (P3HIP_FLAG_FP32) without a GPU: the flag's value, what p3hip_create refuses and what
it plans on the host, the fp32 twin's error against the float64 restatement, the eval player key nn_fp32 and the
resources of the kernels of csrc/conv_f32.hip.

The twin's errors (tests/fp32_common.py twin: float32 torch convolutions, the engine's fp32 BN fold, mish_f, no fp16
rounding) against the float64 restatement, 16 positions, seed 11 (b12c256btl3: its 32 golden positions):
                          raw      probabilities
    test_b3c128btl2       9.4e-7   1.6e-7
    test_b3c256nbt        1.5e-6   1.1e-7
    test_b3c384btl3       1.2e-6   1.1e-7
    test_b3c192classic    1.4e-6   1.3e-7
    test_b5c256btl2_i2    1.6e-6   8.8e-8
    test_b3c96nbt         1.6e-6   1.9e-7
    test_b3c320nbt        1.8e-6   1.6e-7
    test_b4c512btl3_i2    1.3e-6   1.3e-7
    b12c256btl3           4.8e-6   3.0e-7   (against a fixture that stores its float64 outputs as float32)
test_twin_stays_inside_half_of_every_bound re-measures them and asserts that they stay at or below half of the bounds of
tests/fp32_common.py (raw outputs 2e-5, probabilities 1e-6; b12c256btl3 1e-4 and 2e-6)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fp32_common as fc  # noqa: E402
from conftest import ROOT  # noqa: E402

CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("fp32")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = os.path.join(d, name + ".p3w")
            cfg = netspec.get_config(name)
            netspec.save_p3w(cache[name], cfg, netspec.generate_weights(cfg, randomize=True))
        return cache[name]
    return get


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_flag_equals_the_header(built):
    from p3achygo_amd import engine
    text = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    m = re.search(r"^#define P3HIP_FLAG_FP32 (\d+)u", text, re.M)
    assert m and int(m.group(1)) == engine.FLAG_FP32 == 256
    others = [int(v) for v in re.findall(r"^#define P3HIP_FLAG_\w+ (\d+)u", text, re.M)]
    assert others.count(256) == 1   # the bit is the flag's alone


def test_transformers_and_int8_are_refused_before_any_device_call(built, files):
    from p3achygo_amd import engine
    with pytest.raises(engine.EngineError, match="P3HIP_FLAG_FP32"):
        engine.HipEngine(files("test_b2d64h2_tfm"), 4, flags=engine.FLAG_FP32)
    for flag, name in ((engine.FLAG_INT8, "test_b3c384btl3"), (engine.FLAG_INT8, "test_b3c192classic"),
                       (engine.FLAG_INT8_FUSED, "test_b5c256btl2_i2"), (engine.FLAG_INT8_C128, "test_b3c128btl2")):
        with pytest.raises(engine.EngineError, match="P3HIP_FLAG_FP32"):
            engine.HipEngine(files(name), 4, flags=engine.FLAG_FP32 | flag)


@pytest.mark.parametrize("name", fc.SMALL_NETS + [fc.DEEP_NET, fc.OFFSET_NET])
def test_plan_and_weight_images_are_built_on_the_host(built, files, name):
    """without a device p3hip_create fails only at the device: the fp32 plan was built before"""
    from p3achygo_amd import engine
    if _have_gpu():
        pytest.skip("a HIP device is present: creation succeeds (tests/test_fp32_gpu.py)")
    with pytest.raises(engine.EngineError, match="no HIP device"):
        engine.HipEngine(files(name), 4, flags=engine.FLAG_FP32)
    with pytest.raises(engine.EngineError, match="no HIP device"):
        engine.HipEngine(files(name), 4, flags=engine.FLAG_FP32 | engine.FLAG_LAUNCH_GRAPH | engine.FLAG_SYMMETRY_AVG)


@pytest.mark.parametrize("name", fc.SMALL_NETS)
def test_twin_stays_inside_half_of_every_bound(name):
    cfg, W = fc.config(name), fc.weights(name)
    pos = fc.positions()
    raw, prob = fc.errors(fc.outputs(fc.restatement(cfg, W), pos), fc.outputs(fc.twin(cfg, W), pos))
    print(f"fp32 twin {name}: raw {raw:.2e} prob {prob:.2e}")
    assert raw <= fc.RAW_TOL / 2 and prob <= fc.PROB_TOL / 2, (name, raw, prob)


def test_twin_stays_inside_half_of_the_deep_net_bounds():
    cfg, W = fc.config(fc.DEEP_NET), fc.weights(fc.DEEP_NET)
    pos, ref = fc.golden_reference(fc.DEEP_NET)
    raw, prob = fc.errors(ref, fc.outputs(fc.twin(cfg, W), pos))
    print(f"fp32 twin {fc.DEEP_NET}: raw {raw:.2e} prob {prob:.2e}")
    assert raw <= fc.DEEP_RAW_TOL / 2 and prob <= fc.DEEP_PROB_TOL / 2, (raw, prob)


def test_nn_fp32_parses(built, tmp_path):
    from p3achygo_amd import host_api
    H = host_api.lib()
    H.p3host_parse_player_fp32.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_char_p]
    p = tmp_path / "player.cfg"
    val, err = C.c_int(7), C.create_string_buffer(256)
    p.write_text("n: 16\n")
    assert H.p3host_parse_player_fp32(str(p).encode(), C.byref(val), err) == 0 and val.value == 0
    for text, want in (("1", 1), ("0", 0)):
        p.write_text(f"n: 16\nnn_fp32: {text}\n")
        assert H.p3host_parse_player_fp32(str(p).encode(), C.byref(val), err) == 0, (text, err.value)
        assert val.value == want, text
    for text in ("2", "-1", "yes", "true", "0x1", "1.0", "01"):
        p.write_text(f"nn_fp32: {text}\n")
        assert H.p3host_parse_player_fp32(str(p).encode(), C.byref(val), err) == 1, text
        assert b"nn_fp32" in err.value


# ---- kernel resources ------------------------------------------------------------------------------------------------

def _assembly(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = str(tmp_path / "conv_f32_gfx950.s")
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "conv_f32.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return open(out).read()


def test_kernels_spill_nothing_fit_their_lds_and_run_on_the_f32_mfma(tmp_path):
    """from the kernels' metadata: no spills, no private segment, LDS within 80 KiB (every kernel of conv_f32.hip is
    launched two workgroups to a CU); from their text: the f32-input MFMA in every one"""
    asm = _assembly(tmp_path)
    meta = {}
    for blk in re.split(r"^  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):], flags=re.M)[1:]:
        get = lambda key: re.search(r"^    \.%s:\s+(\S+)" % key, blk, re.M).group(1)
        meta[get("name")] = {k: int(get(k)) for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
                                                      "group_segment_fixed_size", "vgpr_count")}
    kinds = sorted(re.search(r"k_\w+?_f32", n).group(0) for n in meta)
    assert kinds == ["k_bdense_f32", "k_init_f32", "k_lconv_f32", "k_lconv_f32"], sorted(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert 0 < m["group_segment_fixed_size"] <= 80 * 1024, (name, m)
        assert m["vgpr_count"] <= 256, (name, m)   # two waves per SIMD
        body = asm[asm.index("\n" + name + ":"):asm.index(".Lfunc_end", asm.index("\n" + name + ":"))]
        assert "v_mfma_f32_32x32x2_f32" in body or "v_mfma_f32_16x16x4_f32" in body, name
