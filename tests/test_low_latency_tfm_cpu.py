"""The low-latency plan of the transformer trunks (P3HIP_FLAG_LOW_LATENCY_TFM, csrc/transformer_split.hip) without a GPU:
the flags' values, the plan p3hip_create chooses and what it refuses (and that P3HIP_FLAG_LOW_LATENCY_ANY on a conv trunk
is P3HIP_FLAG_LOW_LATENCY alone), the chooser of the split (p3hip_debug_tfm_split) against its stated rule, and the
registers, scratch and LDS of every instantiation of the split kernels read from the compiler's assembly."""
import hashlib
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conftest import ROOT  # noqa: E402
from test_plan_matrix_cpu import write_header_file  # noqa: E402

CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")
TFM_NETS = ["test_b2d96h3_tfm", "test_b2d64h2_tfm", "test_b2d128h2_tfm", "test_b2d384h6_tfm"]
CONV_NETS = ["test_b3c256btl1", "test_b3c96nbt"]
PARTS, TOKENS = (1, 2, 3, 6), (16, 32, 64)
SPLITS = [(s, t) for s in PARTS for t in TOKENS]
WIDTHS = [64, 96, 128, 160, 192, 224, 256, 288, 320, 352, 384]
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> .p3w of the net, default-initialised: the plan's path depends on the header alone"""
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("low_latency_tfm")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = os.path.join(d, name + ".p3w")
            if name == "d416h13":   # outside P3HIP_TRANSFORMER_SET: a header and nothing else
                write_header_file(cache[name], 416, 13, 32, 64, 0, 0, "transformer")
            else:
                cfg = netspec.get_config(name)
                netspec.save_p3w(cache[name], cfg, netspec.generate_weights(cfg))
        return cache[name]
    return get


@pytest.fixture()
def env(monkeypatch):
    monkeypatch.delenv("P3HIP_TFM_SPLIT", raising=False)
    monkeypatch.delenv("P3HIP_SPLIT", raising=False)
    return monkeypatch


def _refused(path, flags):
    from p3achygo_amd import engine
    with pytest.raises(engine.EngineError) as ex:
        engine.debug_plan(path, flags)
    msg = str(ex.value)
    assert msg.startswith("p3hip_create: ")   # engine.debug_plan's prefix
    return msg[len("p3hip_create: "):]


def test_flag_values_are_the_headers():
    from p3achygo_amd import engine
    hdr = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    assert re.search(r"#define P3HIP_FLAG_LOW_LATENCY_TFM 8192u", hdr)
    assert re.search(r"#define P3HIP_FLAG_LOW_LATENCY_ANY \(4096u \| 8192u\)", hdr)
    assert engine.FLAG_LOW_LATENCY_TFM == 8192 and engine.FLAG_LOW_LATENCY_ANY == 12288
    assert engine.FLAG_LOW_LATENCY_ANY == engine.FLAG_LOW_LATENCY | engine.FLAG_LOW_LATENCY_TFM


@pytest.mark.parametrize("name", TFM_NETS)
def test_plan_is_tfm_split_with_the_flag_and_tfm_without(built, files, env, name):
    from p3achygo_amd import engine
    assert engine.debug_plan(files(name), 0)[0] == "Tfm"
    for f in (engine.FLAG_LOW_LATENCY_TFM, engine.FLAG_LOW_LATENCY_ANY):
        assert engine.debug_plan(files(name), f) == ("TfmSplit", 0, 0)
        for extra in (engine.FLAG_RUN_ALL_SLOTS, engine.FLAG_SHARED_DEVICE, engine.FLAG_LAUNCH_GRAPH, engine.FLAG_SYMMETRY_AVG,
                      engine.FLAG_AUX):
            assert engine.debug_plan(files(name), extra)[0] == "Tfm"
            assert engine.debug_plan(files(name), f | extra)[0] == "TfmSplit"


@pytest.mark.parametrize("name", CONV_NETS)
def test_both_bits_on_a_conv_trunk_are_low_latency_alone(built, files, env, name):
    from p3achygo_amd import engine
    alone = engine.debug_plan(files(name), engine.FLAG_LOW_LATENCY)
    assert alone[0] == "Split"
    assert engine.debug_plan(files(name), engine.FLAG_LOW_LATENCY_ANY) == alone
    env.setenv("P3HIP_SPLIT", "2,32")
    assert engine.debug_plan(files(name), engine.FLAG_LOW_LATENCY_ANY) == engine.debug_plan(files(name), engine.FLAG_LOW_LATENCY)
    env.setenv("P3HIP_SPLIT", "3,64")   # the conv plan's override stays the conv plan's
    assert "P3HIP_SPLIT" in _refused(files(name), engine.FLAG_LOW_LATENCY_ANY)
    assert engine.debug_plan(files("test_b2d96h3_tfm"), engine.FLAG_LOW_LATENCY_ANY)[0] == "TfmSplit"


def test_refusals(built, files, env):
    from p3achygo_amd import engine
    T, A = engine.FLAG_LOW_LATENCY_TFM, engine.FLAG_LOW_LATENCY_ANY
    for name in CONV_NETS:
        msg = _refused(files(name), T)
        assert "P3HIP_FLAG_LOW_LATENCY_TFM serves the transformer trunks only" in msg, msg
        assert "transformer: d a multiple of 32 with 64 <= d <= 384" in msg       # P3HIP_TRANSFORMER_SET
        assert msg.endswith("the conv trunks have P3HIP_FLAG_LOW_LATENCY"), msg
    for name in TFM_NETS:   # today's text, which the new plan leaves as it is
        msg = _refused(files(name), engine.FLAG_LOW_LATENCY)
        assert "P3HIP_FLAG_LOW_LATENCY serves the conv trunks" in msg and msg.endswith("have no low-latency plan"), msg
    i8 = (engine.FLAG_INT8, engine.FLAG_INT8_FUSED, engine.FLAG_INT8_C128, engine.FLAG_INT8_ANY)
    f32 = (engine.FLAG_FP32, engine.FLAG_FP32_TFM, engine.FLAG_FP32_ANY)
    for name in TFM_NETS[:2]:
        for other in i8 + f32:
            msg = _refused(files(name), T | other)
            assert msg.startswith("P3HIP_FLAG_LOW_LATENCY_TFM cannot be combined with"), msg
            assert ("INT8" if other in i8 else "P3HIP_FLAG_FP32") in msg
            # with P3HIP_FLAG_LOW_LATENCY set as well the clash keeps that flag's text
            assert _refused(files(name), A | other).startswith("P3HIP_FLAG_LOW_LATENCY cannot be combined with")
    for f in (T, A, T | engine.FLAG_AUX):
        assert "unsupported architecture" in _refused(files("d416h13"), f)
    # p3hip_create itself: the same refusals before any device is looked for
    L = engine.lib()
    for path, flags, piece in ((files("test_b3c96nbt"), T, "P3HIP_FLAG_LOW_LATENCY_TFM serves the transformer trunks only"),
                               (files("test_b2d96h3_tfm"), engine.FLAG_LOW_LATENCY, "P3HIP_FLAG_LOW_LATENCY serves the conv trunks"),
                               (files("test_b2d96h3_tfm"), T | engine.FLAG_FP32_TFM, "P3HIP_FLAG_LOW_LATENCY_TFM cannot be combined"),
                               (files("d416h13"), T, "unsupported architecture")):
        assert not L.p3hip_create(path.encode(), 4, 1, 0, flags)
        assert piece in L.p3hip_create_error().decode()


def test_a_bad_override_refuses_the_create_and_only_under_the_flag(built, files, env):
    from p3achygo_amd import engine
    T = engine.FLAG_LOW_LATENCY_TFM
    L = engine.lib()
    for bad in ("4,16", "2,48", "2", "x", "", "2,16,1", "0,64", "6,128"):
        env.setenv("P3HIP_TFM_SPLIT", bad)
        for f in (T, engine.FLAG_LOW_LATENCY_ANY):
            assert "P3HIP_TFM_SPLIT" in _refused(files("test_b2d96h3_tfm"), f)
        assert engine.debug_plan(files("test_b2d96h3_tfm"), 0)[0] == "Tfm"        # without the flag nothing reads it
        assert engine.debug_plan(files("test_b3c96nbt"), engine.FLAG_LOW_LATENCY_ANY)[0] == "Split"
        assert not L.p3hip_create(files("test_b2d96h3_tfm").encode(), 4, 1, 0, T)
        assert "P3HIP_TFM_SPLIT" in L.p3hip_create_error().decode()
    for s, t in SPLITS:
        env.setenv("P3HIP_TFM_SPLIT", "%d,%d" % (s, t))
        assert engine.debug_plan(files("test_b2d96h3_tfm"), T)[0] == "TfmSplit"


def test_create_with_the_flag_fails_only_for_want_of_a_device(built, files, env):
    from p3achygo_amd import engine
    L = engine.lib()
    h = L.p3hip_create(files("test_b2d96h3_tfm").encode(), 4, 1, 0, engine.FLAG_LOW_LATENCY_TFM)
    if h:
        L.p3hip_destroy(h)
    else:
        assert L.p3hip_create_error().decode().startswith("no HIP device")


def _rule(npos, heads, n_cu):
    s = max([p for p in PARTS if npos * heads * p <= n_cu], default=1)
    t = min([t for t in TOKENS if -(-npos * 361 // t) <= n_cu], default=64)
    return s, t


def test_chooser(built, env):
    """inside the kernels' sets; the stated rule (S the largest of {1, 2, 3, 6} with npos x heads x S <= n_cu, T the smallest
    of {16, 32, 64} with ceil(361 npos / T) <= n_cu); monotone (S never grows, T never shrinks with npos); (1, 64) once
    npos x heads > n_cu and ceil(361 npos / 32) > n_cu; the d96h3 thresholds of DESIGN.md section 16"""
    from p3achygo_amd import engine
    n_cu = 256
    for heads in (2, 3, 4, 6, 12):
        prev = None
        for npos in range(1, 2049):
            s, t = engine.debug_tfm_split(npos, heads, n_cu)
            assert s in PARTS and t in TOKENS
            assert (s, t) == _rule(npos, heads, n_cu), (heads, npos, s, t)
            if prev is not None:
                assert s <= prev[0] and t >= prev[1], (heads, npos, prev, (s, t))
            if npos * heads > n_cu and -(-361 * npos // 32) > n_cu:
                assert (s, t) == (1, 64), (heads, npos)
            prev = (s, t)
        assert prev == (1, 64)
    assert engine.debug_tfm_split(1, 3, 256) == (6, 16) == (max(PARTS), min(TOKENS))
    want = {1: (6, 16), 8: (6, 16), 9: (6, 16), 16: (3, 32), 32: (2, 64), 42: (2, 64), 43: (1, 64), 64: (1, 64)}
    for npos, st in want.items():
        assert engine.debug_tfm_split(npos, 3, 256) == st, npos
    assert engine.debug_tfm_split(1, 3, 17) == (3, 32) and engine.debug_tfm_split(1, 3, 5) == (1, 64)   # other devices
    for bad in ((0, 3, 256), (1, 0, 256), (1, 3, 0), (-1, 3, 256)):
        with pytest.raises(ValueError):
            engine.debug_tfm_split(*bad)


def test_chooser_honours_the_override(built, env):
    from p3achygo_amd import engine
    assert len(SPLITS) == 12
    for s, t in SPLITS:
        env.setenv("P3HIP_TFM_SPLIT", "%d,%d" % (s, t))
        for npos in (1, 8, 300, 2048):
            assert engine.debug_tfm_split(npos, 3) == (s, t)
    for bad in ("4,16", "2,48", "2", "x", ""):
        env.setenv("P3HIP_TFM_SPLIT", bad)
        with pytest.raises(ValueError):
            engine.debug_tfm_split(1, 3)
    env.setenv("P3HIP_TFM_SPLIT", "2,32")
    env.setenv("P3HIP_SPLIT", "4,16")   # the conv plan's variable is not this plan's
    assert engine.debug_tfm_split(1, 3) == (2, 32)


def test_player_key_maps_to_both_bits():
    """nn_low_latency: 1 of an eval player asks for the low-latency plan whatever the net's trunk"""
    src = open(os.path.join(ROOT, "p3achygo_amd", "host", "eval_match.cc")).read()
    # written once (EvalEngineFlags), and both engine-opening sites of the match drivers go through it
    assert len(re.findall(r"nn_low_latency \? P3HIP_FLAG_LOW_LATENCY_ANY : 0u", src)) == 1
    assert src.count("EvalEngineFlags(c)") == 1 and src.count("= MakeEvalEvaluator(") == 2
    assert not re.search(r"nn_low_latency \? P3HIP_FLAG_LOW_LATENCY :", src)


# ---- kernel resources (the manner of tests/test_transformer_kernel_resources_cpu.py) ---------------------------------

TFM_CORE = ["transformer_core.h", "transformer_qkv_body.inc", "transformer_attn_body.inc", "transformer_ffn_body.inc"]


def _assembly(stem, sources):
    h = hashlib.sha256()
    for f in sources:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    out = os.path.join(ROOT, "build", "%s_gfx950_%s.s" % (stem, h.hexdigest()[:16]))
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                            os.path.join(CSRC, stem + ".hip"), "-o", out + ".tmp"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + ".tmp", out)
    return open(out).read()


def _kernels(asm, suffix):
    """{("qkv", C, D[, NT]) | ("attn", D) | ("ffn", C[, NT]): dict of the code object's metadata}"""
    res = {}
    for b in asm.split("  - .agpr_count:")[1:]:
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, b).group(1))
        sym = re.search(r"\.name:\s+(\S+)", b).group(1)
        m = re.match(r"_ZN2p312_GLOBAL__N_1\d+k_tfm_(qkv|attn|ffn)%sILi(\d+)E(?:Li(\d+)E)?(?:Li(\d+)E)?EEv" % suffix, sym)
        assert m, sym
        key = (m.group(1),) + tuple(int(x) for x in m.groups()[1:] if x is not None)
        res[key] = dict(vgpr=g("vgpr_count"), lds=g("group_segment_fixed_size"), scratch=g("private_segment_fixed_size"),
                        vspill=g("vgpr_spill_count"), sspill=g("sgpr_spill_count"))
    return res


@pytest.fixture(scope="module")
def split_kernels():
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    asm = _assembly("transformer_split", ["transformer_split.hip", "transformer_split.h", "transformer.h"] + TFM_CORE)
    body = asm[:asm.index(".amdhsa_kernel")]
    assert "scratch_" not in body and "v_mfma_f32_16x16x32_f16" in asm
    return _kernels(asm, "_split")


@pytest.fixture(scope="module")
def default_kernels():
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    return _kernels(_assembly("transformer", ["transformer.hip", "transformer.h"] + TFM_CORE), "")


def test_the_instantiation_set_is_the_expected_one(split_kernels):
    want = {("qkv", c, d, nt) for c in WIDTHS for d in (32, 64) if c % d == 0 for nt in (1, 2)} | \
        {("attn", 32), ("attn", 64)} | {("ffn", c, nt) for c in WIDTHS for nt in (1, 2)}
    assert set(split_kernels) == want and len(want) == 58


def test_no_scratch_no_spills_and_inside_a_cu(split_kernels):
    for key, k in split_kernels.items():
        assert k["scratch"] == 0 and k["vspill"] == 0 and k["sspill"] == 0, (key, k)
        assert k["lds"] <= LDS_PER_CU, (key, k)
        assert k["vgpr"] <= 512, (key, k)


def test_lds_against_the_64_token_twins(split_kernels, default_kernels):
    """the attention stages the same K / V image (55,808 B at D = 32); a 16-token qkv or ffn workgroup holds no more LDS
    than its 64-token twin (a quarter of the token rows), a 32-token one no more either"""
    assert split_kernels[("attn", 32)]["lds"] == 55808 == default_kernels[("attn", 32)]["lds"]
    assert split_kernels[("attn", 64)]["lds"] == default_kernels[("attn", 64)]["lds"]
    for key, k in split_kernels.items():
        if key[0] == "attn":
            continue
        twin = default_kernels[key[:-1]]
        nt = key[-1]
        assert k["lds"] <= twin["lds"], (key, k, twin)
        assert k["lds"] * 4 <= twin["lds"] * nt + 4 * 16, (key, k, twin)   # (x1s[1] of the register form: 4 bytes, padded)


# RoPE's a b + c d leaves the compiler the choice of the product that rides in the fma; transformer_split.hip spells out
# the choice every k_tfm_qkv code object shows (rope4): both products of x'[0] rounded and added, the second product of
# x'[1], x'[2] and x'[3] rounded and the first fused.  The fp32 instructions of a RoPE basic block, registers left out:
ROPE_BLOCK = ("v_pk_mul_f32 R, R, R op_sel:[1,0] op_sel_hi:[0,1]",
              "v_pk_mul_f32 R, R, R",
              "v_mul_f32_e32 R, R, R",
              "v_mul_f32_e32 R, R, R",
              "v_pk_fma_f32 R, R, R, R op_sel:[1,0,0] op_sel_hi:[0,1,1] neg_lo:[0,0,1] neg_hi:[0,0,1]",
              "v_pk_fma_f32 R, R, R, R op_sel_hi:[1,1,0]",
              "v_pk_fma_f32 R, R, R, R op_sel_hi:[1,1,0] neg_lo:[0,0,1] neg_hi:[0,0,1]",
              "v_add_f32_e32 R, R, R")


def test_k_tfm_qkv_still_contracts_rope_the_way_the_split_kernels_spell_out():
    """every instantiation of k_tfm_qkv, each of its four token tiles: the one pattern rope4 restates.  A compiler that
    chooses otherwise changes the default plan's bits, and this file's kernels have to follow it"""
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    asm = _assembly("transformer", ["transformer.hip", "transformer.h"] + TFM_CORE)
    seen = 0
    for m in re.finditer(r"^(_ZN2p3\S*k_tfm_qkv\S*):[^\n]*\n(.*?)\n\s*\.section", asm, re.S | re.M):
        blocks = []
        for blk in re.split(r"\n(?=\.LBB|; %bb)", m.group(2)):
            fp = tuple(re.sub(r"v\[\d+:\d+\]|v\d+", "R", t.strip()) for t in blk.splitlines()
                       if re.match(r"\s*v_(pk_)?(mul|fma|fmac|add|sub)_f32", t))
            if any("neg" in t for t in fp):
                blocks.append(fp)
        assert blocks == [ROPE_BLOCK] * 4, (m.group(1), blocks)
        seen += 1
    assert seen == 17
