"""Fused INT8 blocks of the C = 256 btl trunks (P3HIP_FLAG_INT8_FUSED), without a GPU: the quantized tensors of the
served configs, the architecture check at create, the CPU emulation's own error against the float64 goldens
(tests/int8_block_restatement.py), the teacher-forced block criterion of the GPU test on stand-ins, and the compiled
resources of the block kernel (csrc/block_i8.hip, k_block_i8 at geometry <256,128>)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden  # noqa: E402
import int8_block_restatement as br  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")
REFUSAL = "INT8_FUSED is available only for C = 256 / C_b = 128 trunks of btl blocks"


def _p3w_convs(cfg):
    """(block, conv) of every conv the engine quantizes, read off the weight names of the .p3w generator."""
    from p3achygo_amd import netspec
    W = netspec.generate_weights(cfg, randomize=False)
    out = []
    for k in W:
        m = re.fullmatch(r"blocks\.(\d+)\.conv(\d+)\.w", k)
        if m and cfg.block_kind(int(m.group(1))) != "broadcast":
            out.append((int(m.group(1)), int(m.group(2))))
    return sorted(out)


@pytest.mark.parametrize("name", br.SERVED)
def test_quantized_tensors_of_each_served_config(name):
    from p3achygo_amd import netspec
    cfg = netspec.CONFIGS[name]
    assert br.is_served(cfg)
    names = br.quantized_tensors(cfg)
    n_blocks = sum(cfg.block_kind(i) != "broadcast" for i in range(cfg.blocks))
    assert len(names) == (cfg.inner_layers + 2) * n_blocks
    if name == "b12c256btl3":
        assert len(names) == 50
    assert [tuple(int(v) for v in re.findall(r"\d+", n)) for n in names] == _p3w_convs(cfg)
    # the emulation's calibration visits them in that order, one maximum each
    obs = []
    rng = np.random.default_rng(0)
    W = netspec.generate_weights(cfg, randomize=True)
    br.forward(cfg, W, rng.integers(0, 2, (1, 19, 19, 15)).astype(np.float32), rng.normal(size=(1, 8)).astype(np.float32),
               observe=obs)
    assert len(obs) == len(names) and all(v > 0 for v in obs)


def test_nothing_quantized_outside_the_served_trunks():
    from p3achygo_amd import netspec
    for name in ("test_b3c256nbt", "test_b3c128btl2", "test_b3c384btl3", "b12c128btl3"):
        assert not br.is_served(netspec.CONFIGS[name]) and br.quantized_tensors(netspec.CONFIGS[name]) == []


def test_create_serves_the_c256_btl_trunks_and_refuses_the_rest(built, weight_files, tmp_path):
    """The architecture check comes before the device check: without a GPU the served nets fail only for want of a
    device, everything else with the message that names the served set."""
    from p3achygo_amd import engine, netspec
    import tfm_restatement
    assert engine.FLAG_INT8_FUSED == 64
    header = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    assert re.search(r"#define\s+P3HIP_FLAG_INT8_FUSED\s+64u", header)
    for name in br.SERVED:
        try:
            eng = engine.HipEngine(weight_files(name), 8, flags=engine.FLAG_INT8_FUSED)
        except engine.EngineError as exc:
            assert "no HIP device" in str(exc), (name, str(exc))
        else:
            assert len(eng.int8_scales()) == len(br.quantized_tensors(netspec.CONFIGS[name]))
            eng.close()
    for name in ("test_b3c256nbt", "test_b3c128btl2", "test_b3c384btl3"):
        with pytest.raises(engine.EngineError, match=REFUSAL):
            engine.HipEngine(weight_files(name), 8, flags=engine.FLAG_INT8_FUSED)
    cfg, W = tfm_restatement.fixture_weights("test_b2d96h3_tfm")
    p = str(tmp_path / "tfm.p3w")
    netspec.save_p3w(p, cfg, W)
    with pytest.raises(engine.EngineError, match=REFUSAL):
        engine.HipEngine(p, 8, flags=engine.FLAG_INT8_FUSED)
    for name in ("b12c256btl3", "test_b3c384btl3"):   # both INT8 flags together, whichever flag would serve the trunk
        with pytest.raises(engine.EngineError, match=REFUSAL):
            engine.HipEngine(weight_files(name), 8, flags=engine.FLAG_INT8_FUSED | engine.FLAG_INT8)


def _calibration_inputs(path):
    from oracle import oracle
    net = oracle.OracleNet(path)
    return net, [net.fill_inputs(c) for c in br.calibration_batches()]


@pytest.mark.parametrize("name", br.SERVED)
def test_emulation_error_is_within_half_the_gpu_bounds(built, weight_files, name):
    from p3achygo_amd import netspec
    g, _ = load_golden(name)
    cfg = netspec.CONFIGS[name]
    W = netspec.generate_weights(cfg, randomize=True)
    _, cal = _calibration_inputs(weight_files(name))
    scales = br.minmax_scales(cfg, W, cal)
    assert len(scales) == len(br.quantized_tensors(cfg)) and (scales > 0).all()
    out = br.forward(cfg, W, g["planes"], g["scalars"], scales=scales)
    err = br.errors(out, g)
    fp16 = br.errors(br.forward(cfg, W, g["planes"], g["scalars"]), g)
    print(f"{name}: int8 emulation {err}, fp16 storage alone {fp16}")
    for k, bound in br.BOUNDS[name].items():
        assert err[k] <= 0.5 * bound, (name, k, err)
    # and the INT8 error is real: well above what the fp16 storage alone gives
    assert err["logit"] > 4 * fp16["logit"]
    assert np.array_equal(out["raw"][:, :362].argmax(1), np.asarray(g["raw"])[:, :362].argmax(1))


def test_emulation_keeps_the_argmax_of_the_peaked_policy(built, weight_files):
    from p3achygo_amd import netspec
    g, _ = load_golden("b12c256btl3_peaked")
    cfg = netspec.CONFIGS["b12c256btl3"]
    W = netspec.peak_policy(netspec.generate_weights(cfg, randomize=True), 12.0)
    _, cal = _calibration_inputs(weight_files("b12c256btl3", peak=12.0))
    scales = br.minmax_scales(cfg, W, cal)
    out = br.forward(cfg, W, g["planes"], g["scalars"], scales=scales)
    assert np.array_equal(out["raw"][:, :362].argmax(1), np.asarray(g["raw"])[:, :362].argmax(1))


@pytest.mark.parametrize("name", ["test_b5c256btl2_i2", "b12c256btl3"])
def test_block_criterion_separates_a_faithful_engine_from_one_with_wrong_scales(built, weight_files, name):
    """The GPU test's criterion per btl block, teacher-forced from the same x16: mean |d x| of the engine to the INT8
    emulation over mean |d x| of the engine to the unquantized fp16 block, below 0.5.  A stand-in engine that differs
    from the emulation by rounding noise (the emulation with scales times 1 + 1e-6) stays at or below 0.25; one whose
    scales are off by 1e-3 does not pass."""
    from p3achygo_amd import netspec
    g, _ = load_golden(name)
    cfg = netspec.CONFIGS[name]
    W = netspec.generate_weights(cfg, randomize=True)
    _, cal = _calibration_inputs(weight_files(name))
    scales = br.minmax_scales(cfg, W, cal)
    import trunk_emulation as te
    xs = te.Trunk(cfg, W).trunk(planes=g["planes"][:4], scalars=g["scalars"][:4])
    for k in range(cfg.blocks):
        if cfg.block_kind(k) == "broadcast":
            continue
        x_in = xs[k].numpy()
        sk = br.block_scales(cfg, scales, k)
        emu = br.block(cfg, W, k, x_in, sk)
        fp16 = br.block(cfg, W, k, x_in, None)
        near = br.block(cfg, W, k, x_in, sk * np.float32(1 + 1e-6))
        off = br.block(cfg, W, k, x_in, sk * np.float32(1 + 1e-3))
        ratio = lambda e: float(np.abs(e - emu).mean() / np.abs(e - fp16).mean())
        print(f"{name} block {k}: stand-in {ratio(near):.3f}, scales off by 1e-3 {ratio(off):.3f}")
        assert ratio(near) <= 0.25, (name, k, ratio(near))
        assert ratio(off) > 0.5, (name, k, ratio(off))


def _resources():
    """name -> (VGPRs, scratch bytes, LDS bytes, MFMAs, scratch instructions) of every k_block_i8 of geometry G256 (the
    mangled name carries the geometry struct) in the unit, from the kernel descriptors the build's compiler writes."""
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "block_i8.hip"), "-o", "-"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = r.stdout
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S*k_block_i8\S*G256\S*)\s*$", asm, re.M):
        name = m.group(1)
        desc = asm[m.start():asm.index(".end_amdhsa_kernel", m.start())]
        vg = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", desc).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1))
        start = re.search(r"^" + re.escape(name) + r":", asm, re.M).start()
        body = asm[start:asm.index(".Lfunc_end", start)]
        out[name] = (vg, scratch, lds, body.count("v_mfma_i32_16x16x64_i8"), "scratch_" in body)
    return out


def test_block_kernel_fits_two_waves_per_simd_without_scratch():
    res = _resources()
    assert len(res) == 3, sorted(res)               # one, two and three inner layers
    for name, (vg, scratch, lds, mfma, uses_scratch) in res.items():
        assert scratch == 0 and not uses_scratch, name
        # one 512-thread workgroup per CU = two waves per SIMD: at most 256 VGPRs (arch + acc) a wave
        assert vg <= 256, (name, vg)
        assert lds == 0, (name, lds)                # 112,896 B do not fit a static array: all of it is dynamic LDS
        assert mfma > 0, name
    src = open(os.path.join(CSRC, "block_i8.hip")).read()
    # the CU's workgroups (one at this geometry) within its LDS, and the LDS both images of a position
    assert re.search(r"static_assert\(G::kWgPerCu \* kLdsBytes <= 160 \* 1024", src)
    assert "constexpr int kLdsBytes = (C / 16) * kGroupBytes;" in src and "constexpr int kImgB = (CB / 16) * kGroupBytes;" in src
    assert "static_assert(C == 2 * CB" in src       # so kLdsBytes is two images of kImgB
    assert re.search(r"struct G256 \{ static constexpr int C = 256, CB = 128, kWaves = 8, kWgPerCu = 1; \};", src)
