"""The Winograd plan (P3HIP_FLAG_WINOGRAD) without a GPU: the plan p3hip_create would build and every
refusal by its text, the algorithm against the direct conv in float64, the kernel's weight image, the twin and the
emulation inside the thresholds of tests/winograd_restatement.py, the compiled resources of k_wconv from its code-object
metadata, and the cut of a launch."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_widths_common as cw  # noqa: E402
import winograd_restatement as wr  # noqa: E402
from test_create_matrix_cpu import outcome  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")


def _save(name, directory):
    from p3achygo_amd import netspec
    cfg = netspec.get_config(name)
    path = os.path.join(str(directory), name + ".p3w")
    if not os.path.exists(path):
        netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
    return path


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("winograd")
    return lambda name: _save(name, d)


# ---- 1. the plan ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", wr.NETS)
def test_plan_is_winograd3(built, files, monkeypatch, name):
    """every served kind of trunk: the path is Winograd3 with no quantized tensor, with and without P3HIP_CONV_ANY=1, and
    together with the flags that do not touch the trunk; without the flag the fp16 plan is what it was"""
    from p3achygo_amd import engine
    monkeypatch.delenv("P3HIP_CONV_ANY", raising=False)
    F = engine.FLAG_WINOGRAD
    assert engine.debug_plan(files(name), F) == ("Winograd3", 0, 0)
    assert outcome(files(name), F) == "accepted"
    templated = name in wr.TEMPLATED or name == "test_b3c192classic"
    assert engine.debug_plan(files(name), 0)[0] == ("Layerwise" if templated else "ConvAny")
    for extra in (engine.FLAG_SYMMETRY_SLOT, engine.FLAG_AUX, engine.FLAG_LAUNCH_GRAPH,
                  engine.FLAG_SYMMETRY_SLOT | engine.FLAG_LAUNCH_GRAPH, engine.FLAG_AUX | engine.FLAG_LAUNCH_GRAPH):
        assert engine.debug_plan(files(name), F | extra)[0] == "Winograd3"
        assert outcome(files(name), F | extra) == "accepted"
    monkeypatch.setenv("P3HIP_CONV_ANY", "1")
    assert engine.debug_plan(files(name), F) == ("Winograd3", 0, 0)


def test_every_refusal_names_the_flag(built, files, tmp_path):
    from p3achygo_amd import engine
    F = engine.FLAG_WINOGRAD

    def refused(path, flags, match):
        with pytest.raises(engine.EngineError, match=match) as ex:
            engine.HipEngine(path, 4, flags=flags)
        assert "P3HIP_FLAG_WINOGRAD" in str(ex.value)
        with pytest.raises(engine.EngineError, match=match):
            engine.debug_plan(path, flags)

    tfm = _save("test_b2d64h2_tfm", tmp_path)
    for flags in (F, F | engine.FLAG_INT8, F | engine.FLAG_FP32_TFM, F | engine.FLAG_LOW_LATENCY_TFM):
        refused(tfm, flags, "transformer trunks .* have no 3x3 convs")
    for name in ("test_b3c256btl1", "test_b3c256nbt", "test_b3c128btl2", "test_b3c128nbt"):
        refused(_save(name, tmp_path), F, "run the fused block kernel, and a layer-wise Winograd plan for them is not built")
    lw = files("test_b3c384btl3")
    for other in ("FLAG_INT8", "FLAG_INT8_FUSED", "FLAG_INT8_C128", "FLAG_INT8_ANY", "FLAG_INT8_CONV3"):
        refused(lw, F | getattr(engine, other), "cannot be combined with P3HIP_FLAG_INT8, .* its kernel runs in fp16")
    for other in ("FLAG_FP32", "FLAG_FP32_TFM"):
        refused(lw, F | getattr(engine, other), "cannot be combined with P3HIP_FLAG_FP32 or P3HIP_FLAG_FP32_TFM")
    for other in ("FLAG_LOW_LATENCY", "FLAG_LOW_LATENCY_TFM"):
        refused(lw, F | getattr(engine, other), "cannot be combined with P3HIP_FLAG_LOW_LATENCY or P3HIP_FLAG_LOW_LATENCY_TFM")
    # a clash answers before the trunk does
    refused(_save("test_b3c256btl1", tmp_path), F | engine.FLAG_INT8_FUSED, "cannot be combined with P3HIP_FLAG_INT8")


# ---- 2. the algorithm -------------------------------------------------------------------------------------------------

def test_unrounded_algorithm_is_the_direct_conv():
    """F(2x2, 3x3) over 10 x 10 tiles with zero rows and columns -1, 19, 20 and row / column 19 dropped, in float64 without
    any rounding, against the zero-padded direct 3x3 conv: 1e-12 at every point, rows and columns 0 and 18 included"""
    rng = np.random.default_rng(3)
    a = torch.from_numpy(rng.standard_normal((2, 24, 19, 19)))
    w = rng.standard_normal((3, 3, 24, 40)).astype(np.float32)
    got = wr.wino_conv(a, w, fp16=False)
    want = torch.nn.functional.conv2d(a, torch.from_numpy(w.astype(np.float64)).permute(3, 2, 0, 1), padding=1)
    d = (got - want).abs()
    assert got.shape == want.shape == (2, 40, 19, 19)
    assert float(d.max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    for edge in (d[:, :, 0], d[:, :, 18], d[:, :, :, 0], d[:, :, :, 18]):
        assert float(edge.max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # the twin's order is the same algorithm
    assert float((wr.wino_conv(a, w, fp16=False, other_order=True) - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_input_transform_stages_are_single_fp16_operations():
    """every element of both stages is the fp16 rounding of an exact sum of two fp16 values: numpy's float16 arithmetic,
    operation by operation, gives the same bits"""
    rng = np.random.default_rng(4)
    a16 = (rng.standard_normal((1, 8, 19, 19)) * 3).astype(np.float16)
    v = wr.input_transform(torch.from_numpy(a16.astype(np.float64))).numpy()
    p = np.zeros((1, 8, 22, 22), np.float16)
    p[:, :, 1:20, 1:20] = a16
    for ty, tx in ((0, 0), (0, 9), (9, 0), (9, 9), (4, 5)):
        d = p[:, :, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4]
        t = np.stack([d[:, :, 0] - d[:, :, 2], d[:, :, 1] + d[:, :, 2], d[:, :, 2] - d[:, :, 1], d[:, :, 1] - d[:, :, 3]], 2)
        want = np.stack([t[..., 0] - t[..., 2], t[..., 1] + t[..., 2], t[..., 2] - t[..., 1], t[..., 1] - t[..., 3]], 3)
        assert want.dtype == np.float16
        assert np.array_equal(v[:, :, ty, tx], want.astype(np.float64))


# ---- 3. the weight image ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin,cout,cin_pad,cout_pad", [(32, 64, 64, 64), (96, 128, 128, 128), (24, 40, 64, 64)])
def test_pack_wconv_is_fp16_of_g_g_gt_in_the_documented_layout(built, cin, cout, cin_pad, cout_pad):
    """[cout_pad / 16][cin_pad / 32][16 planes][64 lanes][8] = fp16(G g G^T)[plane / 4][plane % 4][32 k + 8 (lane >> 4) + e]
    [16 ct + (lane & 15)], from the fp32 weights and rounded once; padded rows and columns exactly zero"""
    from p3achygo_amd import engine
    rng = np.random.default_rng(cin)
    w = rng.standard_normal((9, cin, cout)).astype(np.float32)
    img = engine.pack_wconv(w, cin_pad, cout_pad)
    assert img.shape == (cout_pad // 16, cin_pad // 32, 16, 64, 8) and img.dtype == np.float16
    u = np.zeros((4, 4, cin_pad, cout_pad), np.float64)
    u[:, :, :cin, :cout] = wr.transformed_weights(w.reshape(3, 3, cin, cout))
    lane, e = np.meshgrid(np.arange(64), np.arange(8), indexing="ij")
    for ct in range(cout_pad // 16):
        for k in range(cin_pad // 32):
            ci, co = 32 * k + 8 * (lane >> 4) + e, 16 * ct + (lane & 15)
            for p in range(16):
                assert np.array_equal(img[ct, k, p].astype(np.float64), u[p // 4, p % 4, ci, co]), (ct, k, p)
    # the padding, said once more on its own: nothing but zero bits
    full = np.zeros((16, cin_pad, cout_pad), np.uint16)
    for ct in range(cout_pad // 16):
        for k in range(cin_pad // 32):
            full[:, 32 * k + 8 * (lane >> 4) + e, 16 * ct + (lane & 15)] = img[ct, k].view(np.uint16)
    assert not full[:, cin:, :].any() and not full[:, :, cout:].any()
    # from the fp32 weights, not from their fp16 rounding: the two differ somewhere
    u16 = wr.transformed_weights(w.astype(np.float16).astype(np.float32).reshape(3, 3, cin, cout))
    assert not np.array_equal(u16, u[:, :, :cin, :cout])


# ---- 4. the twin and the emulation inside the thresholds --------------------------------------------------------------

@pytest.mark.parametrize("name", wr.NETS)
def test_twin_passes_the_block_thresholds_and_emulation_is_within_a_third_of_the_whole_net_bounds(name):
    """The twin (same storage points, float32 in another order) chained through the net, every block checked from the
    twin's own x as the GPU test checks the engine: inside BLOCK_BOUNDS, and no worse than TWIN records.  The emulation's
    own error to the float64 outputs: what EMULATED records (to its three digits), and WHOLE_NET is three times that."""
    pos = cw.positions()
    fam = wr.twin_stats(name, pos)   # raises outside the bounds
    for kind, (err, ident) in fam.items():
        if kind in wr.TWIN:
            assert err <= wr.TWIN[kind][0] * 1.001 and ident >= wr.TWIN[kind][1] - 0.0005, (name, kind, err, ident)
            # the margin of trunk_emulation.BOUNDS' own kinds: 1.5 - 2 x the twin's worst
            assert 1.5 * wr.TWIN[kind][0] <= wr.BLOCK_BOUNDS[kind][0] <= 2.0 * wr.TWIN[kind][0] + 0.01
    e = wr.emulation_errors(name)
    print(name, fam, e)
    for k, rec in zip(("raw", "prob", "value_prob"), wr.EMULATED[name]):
        assert e[k] <= rec * 1.006, (name, k, e[k], rec)
        bound = wr.WHOLE_NET[name][k]
        assert e[k] <= bound / 3 * 1.0001 and 3 * rec <= bound <= 3 * rec * 1.10, (name, k, e[k], rec, bound)


# ---- 5. kernel resources ----------------------------------------------------------------------------------------------

def test_kernel_resources_from_the_code_object_metadata():
    """Both instantiations of k_wconv (with and without the prologue), from the compiler's amdhsa metadata alone: no
    private segment and no dynamic stack (no scratch), no spilled vector register, 64 KB of static LDS (V), and more than
    256 but at most 512 registers of the unified file, accumulators included: one wave per SIMD, one 256-thread
    workgroup per CU, the occupancy DESIGN.md section 20 states."""
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "conv_wino.hip"), "-o", "-"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    meta = r.stdout[r.stdout.index(".amdgpu_metadata"):r.stdout.index(".end_amdgpu_metadata")]
    kernels = re.split(r"^  - (?=\.agpr_count)", meta, flags=re.M)[1:]
    seen = set()
    for k in kernels:
        f = {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.(\w+):\s+(\S+)\s*$", k, re.M)}
        name = f["name"]
        assert re.fullmatch(r"_ZN2p37k_wconvILb[01]EEEvNS_9WConvArgsE", name), name
        seen.add(name)
        assert int(f["private_segment_fixed_size"]) == 0 and f["uses_dynamic_stack"] == "false", (name, f)
        assert int(f["vgpr_spill_count"]) == 0, (name, f)
        assert int(f["group_segment_fixed_size"]) == 16 * 8 * 32 * 16 == 65536, (name, f)
        assert int(f["max_flat_workgroup_size"]) == 256
        assert 256 < int(f["vgpr_count"]) <= 512 and int(f["agpr_count"]) >= 128, (name, f)
    assert len(seen) == 2


# ---- 6. the cut of a launch -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cout", [64, 128, 192, 512])
def test_grid_hook_is_monotone_covers_every_tile_once_and_honours_n_cu(built, cout):
    from p3achygo_amd import engine
    last = (0, 0)
    for npos in (1, 2, 3, 5, 8, 28, 41, 82, 100, 1024):
        for n_cu in (1, 8, 256, 304):
            grid, units = engine.debug_wconv_grid(npos, cout, n_cu)
            assert 1 <= grid <= n_cu and grid == min(units, n_cu)
            assert units == -(-100 * npos // 32) * (cout // 64)
        grid, units = engine.debug_wconv_grid(npos, cout, 256)
        assert grid >= last[0] and units > last[1]   # more positions: never a smaller grid, always more work
        last = (grid, units)
        if npos > 100:
            continue
        cover = np.zeros((100 * npos, cout // 64), np.int32)
        for u in range(units):
            g, n, t0, nt, c0 = engine.debug_wconv_grid(npos, cout, 256, unit=u)
            assert (g, n) == (grid, units) and 1 <= nt <= 32 and t0 % 32 == 0 and c0 % 64 == 0 and c0 < cout
            assert t0 + nt <= 100 * npos
            cover[t0:t0 + nt, c0 // 64] += 1
        assert (cover == 1).all()
    for bad in ((0, 64, 256), (1, 96, 256), (1, 576, 256), (1, 64, 0)):
        with pytest.raises(ValueError):
            engine.debug_wconv_grid(*bad)
    with pytest.raises(ValueError):
        engine.debug_wconv_grid(1, 64, 256, unit=4)
    # the second-unit batch of the GPU tests follows from the hook
    cfg = wr.config("test_b3c384btl3")
    n2 = wr.second_unit_batch(cfg, 256, lambda n, c: engine.debug_wconv_grid(n, c, 256))
    assert n2 == wr.gpu_batches(cfg)[2] == 28


# ---- 7. the eval host's player key ------------------------------------------------------------------------------------

def test_player_key_nn_winograd(built, tmp_path):
    """nn_winograd: 1 of an eval player parses, and both engine-opening sites of the host pass P3HIP_FLAG_WINOGRAD for it"""
    import ctypes as C
    from p3achygo_amd import host_api
    H = host_api.lib()
    H.p3host_parse_player_winograd.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_char_p]
    val, err = C.c_int(-1), C.create_string_buffer(256)
    p = tmp_path / "player.cfg"
    p.write_text("n: 8\n")
    assert H.p3host_parse_player_winograd(str(p).encode(), C.byref(val), err) == 0 and val.value == 0
    for text, want in (("nn_winograd: 1\n", 1), ("n: 8\nnn_winograd: 0\n", 0), ("nn_winograd: 1\nnn_fp32: 0\n", 1)):
        p.write_text(text)
        assert H.p3host_parse_player_winograd(str(p).encode(), C.byref(val), err) == 0, (text, err.value)
        assert val.value == want
    for text in ("nn_winograd: 2\n", "nn_winograd: yes\n"):
        p.write_text(text)
        assert H.p3host_parse_player_winograd(str(p).encode(), C.byref(val), err) == 1, text
        assert err.value.decode().startswith("nn_winograd must be 0 or 1"), err.value
    # written once (EvalEngineFlags), and both engine-opening sites of the match drivers go through it
    src = open(os.path.join(ROOT, "p3achygo_amd", "host", "eval_match.cc")).read()
    assert src.count("nn_winograd ? P3HIP_FLAG_WINOGRAD : 0u") == 1
    assert src.count("EvalEngineFlags(c)") == 1 and src.count("= MakeEvalEvaluator(") == 2
