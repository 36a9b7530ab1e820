"""The low-latency plan (P3HIP_FLAG_LOW_LATENCY, csrc/conv_split.hip) without a GPU: the plan p3hip_create chooses and
what it refuses, the chooser of the split (p3hip_debug_split), the kernel's weight image against a numpy restatement of
its documented layout, the emulated errors and the twin block check behind the tolerances of
tests/test_low_latency_gpu.py for the nets whose default plan is not layer-wise, the eval player key, and the
registers, scratch and LDS of k_sconv read from the compiler's assembly."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import conv_widths_common as cw  # noqa: E402
import low_latency_common as ll  # noqa: E402
import trunk_emulation as te  # noqa: E402

CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")
PLAN_NETS = {"test_b3c256btl1": "Fused", "test_b3c128nbt": "Fused", "test_b3c384btl3": "Layerwise",
             "test_b3c192classic": "Layerwise", "test_b3c64btl2": "ConvAny", "test_b3c96nbt": "ConvAny",
             "test_b4c512btl3_i2": "ConvAny"}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> .p3w of the net (any table of netspec), default-initialised: the plan depends on the header alone"""
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("low_latency")
    cache = {}

    def get(name):
        if name not in cache:
            cfg = netspec.get_config(name)
            cache[name] = os.path.join(d, name + ".p3w")
            netspec.save_p3w(cache[name], cfg, netspec.generate_weights(cfg))
        return cache[name]
    return get


@pytest.fixture()
def no_split(monkeypatch):
    monkeypatch.delenv("P3HIP_SPLIT", raising=False)
    return monkeypatch


def test_flag_value_is_the_headers():
    from p3achygo_amd import engine
    hdr = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    assert re.search(r"#define P3HIP_FLAG_LOW_LATENCY 4096u", hdr)
    assert engine.FLAG_LOW_LATENCY == ll.FLAG == 4096


@pytest.mark.parametrize("name", sorted(PLAN_NETS))
def test_plan_is_split_with_the_flag_and_unchanged_without(built, files, no_split, name):
    from p3achygo_amd import engine
    assert engine.debug_plan(files(name), engine.FLAG_LOW_LATENCY)[0] == "Split"
    assert engine.debug_plan(files(name), 0)[0] == PLAN_NETS[name]
    # the flags it composes with do not change the path
    for extra in (engine.FLAG_RUN_ALL_SLOTS, engine.FLAG_SHARED_DEVICE, engine.FLAG_LAUNCH_GRAPH, engine.FLAG_SYMMETRY_AVG,
                  engine.FLAG_AUX):
        assert engine.debug_plan(files(name), engine.FLAG_LOW_LATENCY | extra)[0] == "Split"


def test_blockw_is_ignored_under_the_flag(built, files, no_split):
    from p3achygo_amd import engine
    no_split.setenv("P3HIP_BLOCKW", "1")
    assert engine.debug_plan(files("test_b3c256btl1"), 0)[0] == "Blockw"
    assert engine.debug_plan(files("test_b3c256btl1"), engine.FLAG_LOW_LATENCY)[0] == "Split"


def test_refusals_name_the_flag(built, files, no_split):
    from p3achygo_amd import engine
    F = engine.FLAG_LOW_LATENCY

    def refused(name, flags):
        with pytest.raises(engine.EngineError) as ex:
            engine.debug_plan(files(name), flags)
        assert "P3HIP_FLAG_LOW_LATENCY" in str(ex.value), str(ex.value)
        return str(ex.value)
    assert "transformer" in refused("test_b2d96h3_tfm", F)
    for name in ("test_b3c256btl1", "test_b3c384btl3", "test_b3c96nbt"):
        for i8 in (engine.FLAG_INT8, engine.FLAG_INT8_FUSED, engine.FLAG_INT8_C128, engine.FLAG_INT8_ANY):
            assert "INT8" in refused(name, F | i8)
        for f32 in (engine.FLAG_FP32, engine.FLAG_FP32_TFM, engine.FLAG_FP32_ANY):
            assert "P3HIP_FLAG_FP32" in refused(name, F | f32)
    for bad in ("3,16", "2,48", "2", "2,16,1", "x", "0,64", "4,128", ""):
        no_split.setenv("P3HIP_SPLIT", bad)
        assert "P3HIP_SPLIT" in refused("test_b3c96nbt", F)
        assert engine.debug_plan(files("test_b3c96nbt"), 0)[0] == "ConvAny"   # without the flag nothing reads it
    # p3hip_create itself: the same refusal before any device is looked for
    L = engine.lib()
    assert not L.p3hip_create(files("test_b3c96nbt").encode(), 4, 1, 0, F)
    assert "P3HIP_FLAG_LOW_LATENCY" in L.p3hip_create_error().decode()
    for s, t in ll.SPLITS:
        no_split.setenv("P3HIP_SPLIT", "%d,%d" % (s, t))
        assert engine.debug_plan(files("test_b3c96nbt"), F)[0] == "Split"


def test_create_with_the_flag_fails_only_for_want_of_a_device(built, files, no_split):
    from p3achygo_amd import engine
    L = engine.lib()
    h = L.p3hip_create(files("test_b3c96nbt").encode(), 4, 1, 0, engine.FLAG_LOW_LATENCY)
    if h:
        L.p3hip_destroy(h)
    else:
        assert L.p3hip_create_error().decode().startswith("no HIP device")


def test_chooser(built, no_split):
    """inside the kernel's sets, monotone (more positions never give a finer split: strips and tiles-per-64 never grow),
    (1, 64) from some npos on and from npos x cout / 64 >= n_cu at the latest, the finest split at npos = 1 and
    cout = 128, and the rule itself: the finest level of (1, 64), (2, 64), (2, 32), (4, 32), (4, 16) whose items fit one
    round of n_cu workgroups"""
    from p3achygo_amd import engine
    n_cu = 256
    for kw in (1, 3):
        for cout in (64, 128, 192, 256, 512):
            prev = None
            settled = None
            for npos in range(1, 2049):
                s, t = engine.debug_split(npos, kw, cout, n_cu)
                assert (s, t) in ll.SPLITS
                if prev is not None:
                    assert s <= prev[0] and t >= prev[1], (kw, cout, npos, prev, (s, t))
                if (s, t) == (1, 64) and settled is None:
                    settled = npos
                if npos * (cout // 64) >= n_cu:
                    assert (s, t) == (1, 64), (kw, cout, npos)
                levels = [(1, 64), (2, 64), (2, 32), (4, 32), (4, 16)]
                fit = [lv for lv in levels if npos * lv[0] * (cout // lv[1]) <= n_cu]
                assert (s, t) == (fit[-1] if fit else (1, 64)), (kw, cout, npos, s, t)
                prev = (s, t)
            assert settled is not None and settled <= 256
    assert engine.debug_split(1, 3, 128, n_cu) == (4, 16) == (max(s for s, _ in ll.SPLITS), min(t for _, t in ll.SPLITS))
    assert engine.debug_split(1, 1, 128, n_cu) == (4, 16)
    for bad in ((0, 3, 64), (1, 2, 64), (1, 3, 96), (1, 3, 0)):
        with pytest.raises(ValueError):
            engine.debug_split(*bad, n_cu)


def test_chooser_honours_the_override(built, no_split):
    from p3achygo_amd import engine
    for s, t in ll.SPLITS:
        no_split.setenv("P3HIP_SPLIT", "%d,%d" % (s, t))
        for npos in (1, 8, 300, 2048):
            assert engine.debug_split(npos, 3, 128) == (s, t)
    no_split.setenv("P3HIP_SPLIT", "8,64")
    with pytest.raises(ValueError):
        engine.debug_split(1, 3, 128)


@pytest.mark.parametrize("cin,cin_pad,cout", [(48, 64, 64), (160, 192, 320)])
@pytest.mark.parametrize("taps", [1, 9])
def test_pack_sconv_is_the_documented_layout(built, cin, cin_pad, cout, taps):
    """[cout_pad / 16 ct][cin_pad / 32 k][taps][64 lanes][8 e] = W[tap][32 k + 8 (lane >> 4) + e][16 ct + (lane & 15)] in
    fp16, zero where the row or the column is padding (conv_split.h)"""
    from p3achygo_amd import engine
    rng = np.random.default_rng(cin + taps)
    w = rng.standard_normal((taps, cin, cout)).astype(np.float32)
    for cout_pad in (cout, cout + 64):   # padded columns as well as padded rows
        img = engine.pack_sconv(w, cin_pad, cout_pad)
        wp = np.zeros((taps, cin_pad, cout_pad), np.float32)
        wp[:, :cin, :cout] = w
        ct, k, tap, lane, e = np.meshgrid(np.arange(cout_pad // 16), np.arange(cin_pad // 32), np.arange(taps), np.arange(64),
                                          np.arange(8), indexing="ij")
        want = wp[tap, 32 * k + 8 * (lane >> 4) + e, 16 * ct + (lane & 15)].astype(np.float16)
        assert img.shape == want.shape and img.tobytes() == want.tobytes()
        ci = 32 * k + 8 * (lane >> 4) + e
        co = 16 * ct + (lane & 15)
        assert (img[(ci >= cin) | (co >= cout)] == 0).all() and np.abs(img[(ci < cin) & (co < cout)]).min() > 0


@pytest.fixture(scope="module")
def emulated():
    pos = cw.positions()
    out = {}
    for name in ll.FUSED_NETS:
        cfg, W = ll.config(name), ll.weights(name)
        out[name] = cw.emulated_errors(cw.outputs(cfg, W, pos, False), cw.outputs(cfg, W, pos, True))
        print(name, {k: float("%.3g" % v) for k, v in out[name].items()})
    return out


def test_emulated_errors_of_the_fused_default_nets_hold_the_table(emulated):
    """the layer-wise fp16 emulation against the float64 restatement (16 positions, seed 11) on the nets that run fused
    by default: the table of low_latency_common rounds each measurement up by at most a tenth, and every bound of the
    GPU test is at least twice the emulated error (the rule of conv_widths_common.tolerance)"""
    tol = ll.tolerances()
    for name, e in emulated.items():
        for c, v in ll.EMULATED[name].items():
            assert e[c] <= v <= 1.1 * e[c] + 1e-12, (name, c, e[c], v)
        t = tol[name]
        assert (t["logit"] == cw.LOGIT_TOL) == (e["logit_share"] <= 0.5), (name, e)
        assert e["logit"] <= t["logit"] / 2 or e["logit_share"] <= 0.5, (name, e)
        for c in cw.COLUMNS[1:]:
            assert e[c] <= t[c] / 2 and t[c] >= cw.BASE[c], (name, c, e[c], t[c])


def test_twin_of_the_fused_default_nets_is_inside_half_the_layerwise_bounds():
    """the twin block check of tests/test_conv_widths_cpu.py on the four nets: a net keeps a bound of
    trunk_emulation.BOUNDS where its twin's worst error is at most half of it, and overrides it in
    low_latency_common.BLOCK_BOUNDS only where it is not"""
    from test_conv_widths_gpu import block_batch
    pos, slots = block_batch(37)
    for name in ll.FUSED_NETS:
        cfg, W = ll.config(name), ll.weights(name)
        xt = cw.trunk(cfg, W, twin=True).trunk(pos[slots])
        st = cw.teacher_forced(cw.trunk(cfg, W), xt, pos[slots], slots=slots, label=name + " block ",
                               bounds=ll.BLOCK_BOUNDS[name])
        print(name, {k: (round(v["max_err"], 2), round(v["identical"], 3)) for k, v in st.items()})
        worst = {}
        for k, v in st.items():
            key = "stem" if k == "stem" else cw.kind_of(cfg, k)
            max_err, min_identical = ll.BLOCK_BOUNDS[name].get(key, te.BOUNDS[key])
            assert v["max_err"] <= max_err / 2 and v["identical"] >= min_identical, (name, k, key, v)
            worst[key] = max(worst.get(key, 0.0), v["max_err"])
        for key in ll.BLOCK_BOUNDS[name]:   # an override only where the twin passes half of the shared bound
            assert worst[key] > te.BOUNDS[key][0] / 2, (name, key, worst[key])
            assert ll.BLOCK_BOUNDS[name][key][1] == te.BOUNDS[key][1]


def test_player_key_nn_low_latency(built, tmp_path):
    from p3achygo_amd import host_api
    H = host_api.lib()
    H.p3host_parse_player_low_latency.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_char_p]
    val, err = C.c_int(-1), C.create_string_buffer(256)
    p = tmp_path / "player.cfg"
    p.write_text("n: 8\n")
    assert H.p3host_parse_player_low_latency(str(p).encode(), C.byref(val), err) == 0 and val.value == 0
    for text, want in (("nn_low_latency: 1\n", 1), ("n: 8\nnn_low_latency: 0\n", 0), ("nn_low_latency: 1\nnn_fp32: 0\n", 1)):
        p.write_text(text)
        assert H.p3host_parse_player_low_latency(str(p).encode(), C.byref(val), err) == 0, (text, err.value)
        assert val.value == want
    for text in ("nn_low_latency: 2\n", "nn_low_latency: yes\n", "nn_low_latency: -1\n"):
        p.write_text(text)
        assert H.p3host_parse_player_low_latency(str(p).encode(), C.byref(val), err) == 1, text
        assert err.value.decode().startswith("nn_low_latency must be 0 or 1"), err.value


# ---- kernel resources (the manner of tests/test_conv_widths_cpu.py) -------------------------------------------------

def _assembly():
    import shutil
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    h = hashlib.sha256()
    for f in ("conv_split.hip", "conv_split.h", "conv_core.h"):
        h.update(open(os.path.join(CSRC, f), "rb").read())
    out = os.path.join(ROOT, "build", "conv_split_gfx950_%s.s" % h.hexdigest()[:16])
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        for old in os.listdir(os.path.dirname(out)):
            if old.startswith("conv_split_gfx950_") and old.endswith(".s"):
                os.remove(os.path.join(os.path.dirname(out), old))
        r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                            os.path.join(CSRC, "conv_split.hip"), "-o", out + ".tmp"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + ".tmp", out)
    return open(out).read()


def _geo(kw):
    """conv_split.hip GeoS<KW>: (bytes of the activation planes, bytes of the weight fragments)"""
    pad, ksteps = kw // 2, (1 if kw == 3 else 2)
    nslot = (pad + (19 + 2 * pad) * (19 + pad) + pad + 15) // 16 * 16
    return 4 * ksteps * nslot * 16, 4 * ksteps * kw * kw * 1024


def test_k_sconv_uses_no_scratch_and_fits_the_occupancy_design_states():
    """both instantiations, from the code object's metadata: no scratch, the static LDS GeoS gives, and registers
    (VGPRs + AGPRs) and LDS that allow what DESIGN.md section 15 states: one 4-wave workgroup per CU, one wave per SIMD
    (at most 512 registers a lane; the LDS alone would allow two workgroups)"""
    asm = _assembly()
    meta = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", asm, re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        meta[name] = dict(scratch=get("private_segment_fixed_size"), vgprs=get("vgpr_count"), agprs=get("agpr_count"),
                          lds=get("group_segment_fixed_size"), spill=get("vgpr_spill_count"))
    ks = {kw: [v for n, v in meta.items() if "k_sconvILi%dE" % kw in n] for kw in (1, 3)}
    assert len(meta) == 2 and all(len(v) == 1 for v in ks.values()), sorted(meta)
    for kw in (1, 3):
        k = ks[kw][0]
        print("k_sconv<%d>" % kw, k)
        assert k["scratch"] == 0 and k["spill"] == 0, (kw, k)
        assert k["lds"] == sum(_geo(kw)), (kw, k)
        assert k["lds"] <= 64 * 1024                  # static LDS
        assert k["vgprs"] <= 512, (kw, k)             # .vgpr_count counts the unified file: one wave per SIMD
    body = asm[:asm.index(".amdhsa_kernel")] if ".amdhsa_kernel" in asm else asm
    assert "scratch_" not in body and "v_mfma_f32_16x16x32_f16" in body
