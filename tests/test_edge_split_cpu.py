"""The split stem, broadcast dense and heads of the low-latency plans (csrc/edge_split.hip) without a
GPU: the chooser (p3hip_debug_edge_split) and its P3HIP_EDGE_SPLIT override, the refusal of a value outside the sets, the
plans with and without the variable, and the registers, scratch and LDS of the new kernels read from the code object's
metadata."""
import hashlib
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")
WIDTHS = (64, 128, 256, 384, 512)
DENSE, HEADS = (1, 3, 12), (1, 4, 8)          # the documented sets (csrc/edge_split.h)
PLAN_NETS = {"test_b3c64btl2": "ll", "test_b3c128btl2": "ll", "test_b3c256nbt": "ll", "test_b4c512btl3_i2": "ll",
             "test_b2d384h6_tfm": "tfm", "test_b2d96h3_tfm": "tfm"}


def passes(c_pad):
    """output passes of the stem: the stem's parts are 1 or this"""
    return c_pad // (128 if c_pad % 128 == 0 else 64)


@pytest.fixture()
def env(monkeypatch):
    monkeypatch.delenv("P3HIP_EDGE_SPLIT", raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> .p3w of the net, default-initialised: the plan depends on the header alone"""
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("edge_split")
    cache = {}

    def get(name):
        if name not in cache:
            cfg = netspec.get_config(name)
            cache[name] = os.path.join(d, name + ".p3w")
            netspec.save_p3w(cache[name], cfg, netspec.generate_weights(cfg))
        return cache[name]
    return get


def test_hook_is_exported_and_declared(built):
    from p3achygo_amd import engine
    hdr = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    assert "p3hip_debug_edge_split" in engine.EXPORTS and re.search(r"\bint p3hip_debug_edge_split\(", hdr)
    assert "P3HIP_EDGE_SPLIT" in hdr


def test_chooser(built, env):
    """npos 1 .. 300, every width, 64 and 256 CUs: parts from the documented sets; whenever a piece is split its items
    (positions x parts; the dense: x the 128-channel halves) fit one round of the CUs, and the split is the finest level
    that does; parts never grow with npos; all three are 1 from some npos on"""
    from p3achygo_amd import engine
    for n_cu in (64, 256):
        for c_pad in WIDTHS:
            nhalf = (c_pad + 127) // 128
            prev, settled = None, None
            for npos in range(1, 301):
                s, d, h = engine.debug_edge_split(npos, c_pad, n_cu)
                assert s in (1, passes(c_pad)) and d in DENSE and h in HEADS, (n_cu, c_pad, npos, s, d, h)
                assert s == 1 or npos * s <= n_cu
                assert d == 1 or npos * nhalf * d <= n_cu
                assert h == 1 or npos * h <= n_cu
                # the finest level that fits
                assert s == (passes(c_pad) if npos * passes(c_pad) <= n_cu else 1)
                assert d == max([x for x in DENSE if npos * nhalf * x <= n_cu] or [1])
                assert h == max([x for x in HEADS if npos * x <= n_cu] or [1])
                if prev is not None:
                    assert s <= prev[0] and d <= prev[1] and h <= prev[2], (n_cu, c_pad, npos, prev, (s, d, h))
                if (s, d, h) == (1, 1, 1):
                    settled = settled or npos
                else:
                    assert settled is None
                prev = (s, d, h)
            assert settled is not None and settled <= 300, (n_cu, c_pad)
    assert engine.debug_edge_split(1, 512) == (4, 12, 8) and engine.debug_edge_split(8, 256) == (2, 12, 8)


def test_bad_arguments_answer_1(built, env):
    import ctypes as C
    from p3achygo_amd import engine
    L = engine.lib()
    L.p3hip_debug_edge_split.argtypes = [C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 3
    for npos, c_pad, n_cu in ((0, 256, 256), (-3, 256, 256), (1, 0, 256), (1, 96, 256), (1, 576, 256), (1, 256, 0)):
        s, d, h = C.c_int(9), C.c_int(9), C.c_int(9)
        assert L.p3hip_debug_edge_split(npos, c_pad, n_cu, C.byref(s), C.byref(d), C.byref(h)) == 1
        assert (s.value, d.value, h.value) == (1, 1, 1)
        with pytest.raises(ValueError):
            engine.debug_edge_split(npos, c_pad, n_cu)
    assert L.p3hip_debug_edge_split(1, 256, 256, None, None, None) == 1


def test_override_is_honoured(built, env):
    from p3achygo_amd import engine
    for c_pad in WIDTHS:
        for s in sorted({1, passes(c_pad)}):
            for d in DENSE:
                for h in HEADS:
                    env.setenv("P3HIP_EDGE_SPLIT", "%d,%d,%d" % (s, d, h))
                    for npos in (1, 8, 300, 2048):
                        assert engine.debug_edge_split(npos, c_pad) == (s, d, h)
    env.setenv("P3HIP_EDGE_SPLIT", "0")
    for c_pad in WIDTHS:
        for npos in (1, 8, 300):
            assert engine.debug_edge_split(npos, c_pad) == (1, 1, 1)
    # outside the sets; a stem count that is not this width's passes
    for bad in ("1,2,1", "1,3,2", "1,3", "1,3,4,1", "x", "", "0,3,4", "1,3,16", "00", "1,1,1 "):
        env.setenv("P3HIP_EDGE_SPLIT", bad)
        with pytest.raises(ValueError):
            engine.debug_edge_split(1, 256)
    env.setenv("P3HIP_EDGE_SPLIT", "2,3,4")
    assert engine.debug_edge_split(1, 256) == (2, 3, 4)
    for c_pad in (64, 128, 384, 512):
        with pytest.raises(ValueError):
            engine.debug_edge_split(1, c_pad)


@pytest.mark.parametrize("name", sorted(PLAN_NETS))
def test_plan_and_refusals(built, files, env, name):
    """the path, the quantized tensors and the digest are the same with and without P3HIP_EDGE_SPLIT (only launches
    differ); a value outside the sets fails the create with a message that names the variable, before any device is
    looked for; without a low-latency flag nothing reads it"""
    from p3achygo_amd import engine, netspec
    F = engine.FLAG_LOW_LATENCY if PLAN_NETS[name] == "ll" else engine.FLAG_LOW_LATENCY_TFM
    cfg = netspec.get_config(name)
    c_pad = (cfg.channels + 63) // 64 * 64 if PLAN_NETS[name] == "ll" else (128 if cfg.channels <= 128 else 384)
    want = engine.debug_plan(files(name), F)
    assert want[0] == ("Split" if PLAN_NETS[name] == "ll" else "TfmSplit")
    plain = engine.debug_plan(files(name), 0)
    for ok in ["0"] + ["%d,%d,%d" % (s, d, h) for s in sorted({1, passes(c_pad)}) for d in DENSE for h in HEADS]:
        env.setenv("P3HIP_EDGE_SPLIT", ok)
        assert engine.debug_plan(files(name), F) == want, ok
        assert engine.debug_plan(files(name), F | engine.FLAG_LAUNCH_GRAPH) == want
    L = engine.lib()
    for bad in ("1,2,1", "1,3,2", "7,1,1", "1,3", "x", "", "%d,1,1" % (passes(c_pad) + 1)):
        env.setenv("P3HIP_EDGE_SPLIT", bad)
        with pytest.raises(engine.EngineError) as ex:
            engine.debug_plan(files(name), F)
        assert "P3HIP_EDGE_SPLIT" in str(ex.value), str(ex.value)
        assert not L.p3hip_create(files(name).encode(), 4, 1, 0, F)
        assert "P3HIP_EDGE_SPLIT" in L.p3hip_create_error().decode()
        assert engine.debug_plan(files(name), 0) == plain   # without the flag nothing reads it
    # a good value: the create fails only for want of a device
    env.setenv("P3HIP_EDGE_SPLIT", "0")
    h = L.p3hip_create(files(name).encode(), 4, 1, 0, F)
    if h:
        L.p3hip_destroy(h)
    else:
        assert L.p3hip_create_error().decode().startswith("no HIP device")


# ---- kernel resources (the manner of tests/test_low_latency_cpu.py) ---------------------------------------------------

def _assembly():
    import shutil
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    h = hashlib.sha256()
    for f in ("edge_split.hip", "edge_split.h", "layer_kernels.h", "conv_core.h", "kernels.h", "launch_util.h",
              "stem_planes.inc", "stem_epilogue.inc", "bdense_epilogue.inc", "bdense_transpose.inc", "heads_score_bin.inc"):
        h.update(open(os.path.join(CSRC, f), "rb").read())
    out = os.path.join(ROOT, "build", "edge_split_gfx950_%s.s" % h.hexdigest()[:16])
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        for old in os.listdir(os.path.dirname(out)):
            if old.startswith("edge_split_gfx950_") and old.endswith(".s"):
                os.remove(os.path.join(os.path.dirname(out), old))
        r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                            os.path.join(CSRC, "edge_split.hip"), "-o", out + ".tmp"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + ".tmp", out)
    return open(out).read()


def test_new_kernels_use_no_scratch_and_fit_their_launchers_lds():
    """all six kernels, from the code object's metadata: no scratch, no spills; the kernels on dynamic LDS declare no
    static LDS and their launchers' requests (restated here from edge_split.hip) fit a CU's 160 KB, two workgroups of the
    stem at a time; the heads kernels' static LDS is far below the 64 KB a launch gets without asking"""
    asm = _assembly()
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", asm, re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        meta[name] = dict(scratch=get("private_segment_fixed_size"), vgprs=get("vgpr_count"), lds=get("group_segment_fixed_size"),
                          spill=get("vgpr_spill_count"), sspill=get("sgpr_spill_count"), wg=get("max_flat_workgroup_size"))

    def one(pattern):
        hit = [v for n, v in meta.items() if re.search(pattern, n)]
        assert len(hit) == 1, (pattern, sorted(meta))
        return hit[0]
    ks = {"k_init_split<128>": one(r"k_init_splitILi128E"), "k_init_split<64>": one(r"k_init_splitILi64E"),
          "k_bdense_split": one(r"k_bdense_split"), "k_heads_pool": one(r"k_heads_pool"),
          "k_heads_points": one(r"k_heads_points"), "k_heads_softmax": one(r"k_heads_softmax")}
    assert len(meta) == 6, sorted(meta)
    for n, k in ks.items():
        print(n, k)
        assert k["scratch"] == 0 and k["spill"] == 0 and k["sspill"] == 0, (n, k)
    # Geo<1, 16, 5>: slots of 48 bytes, 2 x (2 x 21 + 2) pad slots around 18 x 21 + 19 rows
    act = ((2 * (2 * 21 + 2) + 18 * 21 + 19) * 48 + 15) // 16 * 16
    ring = lambda cp: 3 * 4 * cp * 32
    for cp in (64, 128):
        k = ks["k_init_split<%d>" % cp]
        assert k["lds"] == 0 and k["wg"] == 512 and k["vgprs"] <= 256           # two waves per SIMD
        assert 2 * (act + ring(cp) + cp * 4) <= 160 * 1024
    k = ks["k_bdense_split"]
    assert k["lds"] == 0 and k["wg"] == 512 and k["vgprs"] <= 256
    assert 128 * 784 + ring(128) + (384 + 2 * 512) * 4 <= 160 * 1024
    for n in ("k_heads_pool", "k_heads_points", "k_heads_softmax"):
        assert ks[n]["wg"] == 256 and ks[n]["lds"] <= 4096 and ks[n]["vgprs"] <= 128, (n, ks[n])
    body = asm[:asm.index(".amdhsa_kernel")] if ".amdhsa_kernel" in asm else asm
    assert "scratch_" not in body and "v_mfma_f32_32x32x16_f16" in body
