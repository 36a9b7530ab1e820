"""The fp32 plan of the transformer trunks (P3HIP_FLAG_FP32_TFM) without a GPU: the flags' values, what p3hip_create
refuses and what it plans on the host, the fp32 twin's error against the float64 restatement, the eval player key nn_fp32
and the resources of the kernels of csrc/transformer_f32.hip.

The twin's errors (tests/tfm_fp32_common.py Twin: the three stages, the stem and the heads in float32 torch, no fp16
rounding) against the float64 restatement tests/tfm_restatement_dh.py, on the 16 positions of each fixture
(b14d96h3_transformer: the first 8 of test_b2d96h3_tfm):
                            raw       probabilities
    test_b2d64h2_tfm        3.9e-6    4.3e-7
    test_b2d96h3_tfm        1.15e-5   6.9e-7
    test_b2d128h2_tfm       5.7e-6    3.7e-7
    test_b2d192h6_tfm       8.7e-6    5.1e-7
    test_b2d256h4_tfm       6.1e-6    4.8e-7
    test_b2d384h12_tfm      8.6e-6    6.4e-7
    test_b2d384h6_tfm       8.8e-6    5.0e-7
    b14d96h3_transformer    1.22e-5   7.0e-7
The bounds are twice the worst of each group rounded up to one significant digit (tfm_fp32_common.rule): raw 3e-5 and
probabilities 2e-6 for the seven two-block nets (2 x 1.15e-5 = 2.3e-5, 2 x 6.9e-7 = 1.4e-6) and the same for
b14d96h3_transformer (2.4e-5, 1.4e-6).  The twin tests re-measure the figures, hold them to half of the bounds and check
that the rule applied to them does not ask for more than the bounds the GPU test uses."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tfm_fp32_common as tc  # noqa: E402
from conftest import ROOT  # noqa: E402

CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")
CONV_NET = "test_b3c128btl2"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("tfm_fp32")
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


def test_flags_equal_the_header(built):
    from p3achygo_amd import engine
    text = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    m = re.search(r"^#define P3HIP_FLAG_FP32_TFM (\d+)u", text, re.M)
    assert m and int(m.group(1)) == engine.FLAG_FP32_TFM == 512
    others = [int(v) for v in re.findall(r"^#define P3HIP_FLAG_\w+ (\d+)u", text, re.M)]
    assert others.count(512) == 1 and all(v & 512 == 0 for v in others if v != 512)   # the bit is the flag's alone
    m = re.search(r"^#define P3HIP_FLAG_FP32_ANY \((\d+)u \| (\d+)u\)", text, re.M)
    assert m and int(m.group(1)) | int(m.group(2)) == engine.FLAG_FP32_ANY == 768
    assert engine.FLAG_FP32_ANY == engine.FLAG_FP32 | engine.FLAG_FP32_TFM


def test_conv_trunks_and_int8_are_refused_before_any_device_call(built, files):
    from p3achygo_amd import engine
    with pytest.raises(engine.EngineError, match="P3HIP_FLAG_FP32_TFM") as exc:
        engine.HipEngine(files(CONV_NET), 4, flags=engine.FLAG_FP32_TFM)
    assert "conv trunks have P3HIP_FLAG_FP32" in str(exc.value)
    with pytest.raises(engine.EngineError, match="P3HIP_FLAG_FP32_TFM cannot be combined"):
        engine.HipEngine(files("test_b2d64h2_tfm"), 4, flags=engine.FLAG_FP32_TFM | engine.FLAG_INT8)
    with pytest.raises(engine.EngineError, match="cannot be combined"):
        engine.HipEngine(files(CONV_NET), 4, flags=engine.FLAG_FP32_ANY | engine.FLAG_INT8_C128)
    # P3HIP_FLAG_FP32 alone on a transformer: refused as before, and the message now points to the transformers' flag
    with pytest.raises(engine.EngineError, match="P3HIP_FLAG_FP32 serves the conv trunks only") as exc:
        engine.HipEngine(files("test_b2d64h2_tfm"), 4, flags=engine.FLAG_FP32)
    assert "P3HIP_FLAG_FP32_TFM" in str(exc.value)


@pytest.mark.parametrize("name", tc.NETS + [tc.DEEP_NET])
def test_plan_and_weight_images_are_built_on_the_host(built, files, name):
    """without a device p3hip_create fails only at the device: the fp32 plan was built before"""
    from p3achygo_amd import engine
    if _have_gpu():
        pytest.skip("a HIP device is present: creation succeeds (tests/test_transformer_fp32_gpu.py)")
    extra = engine.FLAG_LAUNCH_GRAPH | engine.FLAG_SYMMETRY_AVG
    for flags in (engine.FLAG_FP32_TFM, engine.FLAG_FP32_TFM | extra):
        with pytest.raises(engine.EngineError, match="no HIP device"):
            engine.HipEngine(files(name), 4, flags=flags)


@pytest.mark.parametrize("name", [CONV_NET, "test_b2d192h6_tfm"])
def test_fp32_any_plans_whatever_the_trunk(built, files, name):
    from p3achygo_amd import engine
    if _have_gpu():
        pytest.skip("a HIP device is present: creation succeeds (tests/test_transformer_fp32_gpu.py)")
    extra = engine.FLAG_LAUNCH_GRAPH | engine.FLAG_SYMMETRY_AVG
    for flags in (engine.FLAG_FP32_ANY, engine.FLAG_FP32_ANY | extra):
        with pytest.raises(engine.EngineError, match="no HIP device"):
            engine.HipEngine(files(name), 4, flags=flags)


def test_nn_fp32_parses(built, tmp_path):
    from p3achygo_amd import host_api
    H = host_api.lib()
    H.p3host_parse_player_fp32.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_char_p]
    p = tmp_path / "player.cfg"
    val, err = C.c_int(7), C.create_string_buffer(256)
    for text, want in (("n: 16\n", 0), ("n: 16\nnn_fp32: 1\n", 1), ("n: 16\nnn_fp32: 0\n", 0)):
        p.write_text(text)
        assert H.p3host_parse_player_fp32(str(p).encode(), C.byref(val), err) == 0 and val.value == want, text
    # written once (EvalEngineFlags), and both engine-opening sites of the match drivers go through it
    src = open(os.path.join(ROOT, "p3achygo_amd", "host", "eval_match.cc")).read()
    assert src.count("nn_fp32 ? P3HIP_FLAG_FP32_ANY") == 1 and "nn_fp32 ? P3HIP_FLAG_FP32 " not in src
    assert src.count("EvalEngineFlags(c)") == 1 and src.count("= MakeEvalEvaluator(") == 2


# ---- the twin ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def twin_errors():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = tc.twin_errors(name)
            print(f"fp32 twin {name}: raw {cache[name][0]:.2e} prob {cache[name][1]:.2e}")
        return cache[name]
    return get


@pytest.mark.parametrize("name", tc.NETS + [tc.DEEP_NET])
def test_twin_stays_inside_half_of_every_bound(twin_errors, name):
    raw, prob = twin_errors(name)
    raw_tol, prob_tol = tc.tolerances(name)
    assert raw <= raw_tol / 2 and prob <= prob_tol / 2, (name, raw, prob)


def test_bounds_are_twice_the_twins_worst(twin_errors):
    """tfm_fp32_common.rule on the re-measured figures stays inside the bounds the GPU test uses"""
    small = [twin_errors(n) for n in tc.NETS]
    deep = twin_errors(tc.DEEP_NET)
    got = (tc.rule(max(e[0] for e in small)), tc.rule(max(e[1] for e in small)), tc.rule(deep[0]), tc.rule(deep[1]))
    print("rule on the re-measured twin: raw %.0e prob %.0e, deep raw %.0e prob %.0e" % got)
    assert all(g <= t * (1 + 1e-9) for g, t in zip(got, (tc.RAW_TOL, tc.PROB_TOL, tc.DEEP_RAW_TOL, tc.DEEP_PROB_TOL))), got


# ---- kernel resources ------------------------------------------------------------------------------------------------

def test_kernels_spill_nothing_fit_their_lds_and_run_on_the_f32_mfma(tmp_path):
    """from the kernels' metadata: no spills, no private segment, LDS within 160 KiB; from their text: the f32-input
    MFMA in every one, and neither an f16-input MFMA nor a conversion between f16 and f32 in any"""
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = str(tmp_path / "transformer_f32_gfx950.s")
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "transformer_f32.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = open(out).read()
    meta = {}
    for blk in re.split(r"^  - \.agpr_count:", asm[asm.index("amdhsa.kernels:"):], flags=re.M)[1:]:
        get = lambda key: re.search(r"^    \.%s:\s+(\S+)" % key, blk, re.M).group(1)
        meta[get("name")] = {k: int(get(k)) for k in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
                                                      "group_segment_fixed_size", "vgpr_count")}
    kinds = sorted(set(re.search(r"k_tfm_\w+?_f32", n).group(0) for n in meta))
    assert kinds == ["k_tfm_attn_f32", "k_tfm_ffn_f32", "k_tfm_qkv_f32"], sorted(meta)
    assert len(meta) == 11 + 2 + 11   # qkv and ffn per model width, attn per head width
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert 0 < m["group_segment_fixed_size"] <= 160 * 1024, (name, m)
        assert m["vgpr_count"] <= 256, (name, m)   # two waves per SIMD: 256 threads are one wave per SIMD, x 2 workgroups
        body = asm[asm.index("\n" + name + ":"):asm.index(".Lfunc_end", asm.index("\n" + name + ":"))]
        assert "v_mfma_f32_32x32x2_f32" in body or "v_mfma_f32_16x16x4_f32" in body, name
        assert not re.search(r"v_mfma_\w*f16", body), name
        assert not re.search(r"v_cvt_f16_f32|v_cvt_f32_f16|v_cvt_pk\w*f16", body), name
