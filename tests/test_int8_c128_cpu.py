"""Fused INT8 blocks of the C = 128 / C_b = 64 btl trunks (P3HIP_FLAG_INT8_C128), without a GPU: the flag, the
architecture check at create, the quantized tensors of the served configs, the CPU emulation's own error against the
float64 goldens (tests/int8_block_c128.py), the teacher-forced block criterion of the GPU test on stand-ins at this
width, and the compiled resources of the block kernel (csrc/block_i8.hip, k_block_i8 at geometry <128,64>)."""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden  # noqa: E402
import int8_block_c128 as bc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")
REFUSAL = "INT8_C128 is available only for C = 128 / C_b = 64 trunks of btl blocks"
REFUSAL_FUSED = "INT8_FUSED is available only for C = 256 / C_b = 128 trunks of btl blocks"


def test_flag_value_in_the_header_and_the_mirror():
    from p3achygo_amd import engine
    assert engine.FLAG_INT8_C128 == 128
    header = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    assert re.search(r"#define\s+P3HIP_FLAG_INT8_C128\s+128u", header)
    flags = [getattr(engine, n) for n in dir(engine) if n.startswith("FLAG_")]
    assert len(set(flags)) == len(flags)   # a bit of its own


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


@pytest.mark.parametrize("name", bc.SERVED + ("b10c128btl3", "small"))
def test_quantized_tensors_follow_the_p3w_conv_order(name):
    from p3achygo_amd import netspec
    cfg = netspec.CONFIGS[name]
    assert bc.is_served(cfg)
    names = bc.quantized_tensors(cfg)
    n_blocks = sum(cfg.block_kind(i) != "broadcast" for i in range(cfg.blocks))
    assert len(names) == (cfg.inner_layers + 2) * n_blocks
    if name == "b12c128btl3":
        assert len(names) == 50
    assert [tuple(int(v) for v in re.findall(r"\d+", n)) for n in names] == _p3w_convs(cfg)
    if name in bc.SERVED:   # the emulation's calibration visits them in that order, one maximum each
        obs = []
        rng = np.random.default_rng(0)
        W = netspec.generate_weights(cfg, randomize=True)
        bc.forward(cfg, W, rng.integers(0, 2, (1, 19, 19, 15)).astype(np.float32),
                   rng.normal(size=(1, 8)).astype(np.float32), observe=obs)
        assert len(obs) == len(names) and all(v > 0 for v in obs)


def test_nothing_quantized_outside_the_served_trunks():
    from p3achygo_amd import netspec
    for name in ("test_b3c128nbt", "b8c128nbt", "test_b3c256btl1", "test_b3c384btl3", "b12c256btl3"):
        assert not bc.is_served(netspec.CONFIGS[name]) and bc.quantized_tensors(netspec.CONFIGS[name]) == []


def test_create_serves_the_c128_btl_trunks_and_refuses_the_rest(built, weight_files, tmp_path):
    """The architecture check comes before the device check: without a GPU the served nets fail only for want of a
    device, everything else with the message that names the served set."""
    from p3achygo_amd import engine, netspec
    import tfm_restatement
    for name in bc.SERVED:
        try:
            eng = engine.HipEngine(weight_files(name), 8, flags=engine.FLAG_INT8_C128)
        except engine.EngineError as exc:
            assert "no HIP device" in str(exc), (name, str(exc))
        else:
            assert len(eng.int8_scales()) == len(bc.quantized_tensors(netspec.CONFIGS[name]))
            eng.close()
    for name in ("test_b3c128nbt", "test_b3c256btl1", "test_b3c384btl3", "b15c192_classic"):
        with pytest.raises(engine.EngineError, match=REFUSAL) as exc:
            engine.HipEngine(weight_files(name), 8, flags=engine.FLAG_INT8_C128)
        assert "b12c128btl3" in str(exc.value) and "no HIP device" not in str(exc.value)
    # a classic trunk of this very width (it runs through the runtime-width kernels) and a transformer
    ccfg = netspec.WIDE_CONV_CONFIGS["test_b3c128classic"]
    tcfg, tW = tfm_restatement.fixture_weights("test_b2d96h3_tfm")
    for fname, cfg, W in (("classic.p3w", ccfg, netspec.generate_weights(ccfg, randomize=True)), ("tfm.p3w", tcfg, tW)):
        p = str(tmp_path / fname)
        netspec.save_p3w(p, cfg, W)
        with pytest.raises(engine.EngineError, match=REFUSAL):
            engine.HipEngine(p, 8, flags=engine.FLAG_INT8_C128)
    # any two of the three INT8 flags (and all three), whichever flag would serve the trunk
    i8 = (engine.FLAG_INT8, engine.FLAG_INT8_FUSED, engine.FLAG_INT8_C128)
    sets = [a | b for a, b in itertools.combinations(i8, 2)] + [i8[0] | i8[1] | i8[2]]
    for name in ("b12c128btl3", "b12c256btl3", "test_b3c384btl3"):
        for flags in sets:
            want = REFUSAL if flags & engine.FLAG_INT8_C128 else REFUSAL_FUSED
            with pytest.raises(engine.EngineError, match=want) as exc:
                engine.HipEngine(weight_files(name), 8, flags=flags)
            assert "not together with" in str(exc.value)


def _calibration_inputs(path):
    from oracle import oracle
    net = oracle.OracleNet(path)
    return net, [net.fill_inputs(c) for c in bc.calibration_batches()]


_EMU = {}


def _emulated(name, weight_files):
    """(cfg, W, scales) of a served fixture: one calibration of the emulation per session."""
    if name not in _EMU:
        from p3achygo_amd import netspec
        cfg = netspec.CONFIGS[name]
        W = netspec.generate_weights(cfg, randomize=True)
        _, cal = _calibration_inputs(weight_files(name))
        _EMU[name] = (cfg, W, bc.minmax_scales(cfg, W, cal))
    return _EMU[name]


@pytest.mark.parametrize("name", bc.SERVED)
def test_emulation_error_is_within_half_the_gpu_bounds(built, weight_files, name):
    g, _ = load_golden(name)
    cfg, W, scales = _emulated(name, weight_files)
    assert len(scales) == len(bc.quantized_tensors(cfg)) and (scales > 0).all()
    out = bc.forward(cfg, W, g["planes"], g["scalars"], scales=scales)
    err = bc.errors(out, g)
    fp16 = bc.errors(bc.forward(cfg, W, g["planes"], g["scalars"]), g)
    print(f"{name}: int8 emulation {err}, fp16 storage alone {fp16}")
    for k, bound in bc.BOUNDS[name].items():
        assert err[k] <= 0.5 * bound, (name, k, err)
    # and the INT8 error is real: well above what the fp16 storage alone gives
    assert err["logit"] > 4 * fp16["logit"]
    if name == "b12c128btl3":   # the full-size net keeps float64's move on every fixture position
        assert np.array_equal(out["raw"][:, :362].argmax(1), np.asarray(g["raw"])[:, :362].argmax(1))


@pytest.mark.parametrize("name", ["test_b5c128btl1_i2", "b12c128btl3"])
def test_block_criterion_separates_a_faithful_engine_from_one_with_wrong_scales(built, weight_files, name):
    """The GPU test's criterion per btl block, teacher-forced from the same x16: mean |d x| of the engine to the INT8
    emulation over mean |d x| of the engine to the unquantized fp16 block, at most 0.5.  A stand-in engine that differs
    from the emulation by rounding noise (the emulation with scales times 1 + 1e-6) stays at or below 0.25, half the
    bound; one whose scales are off by 1e-3 lands as far from the emulation as from the fp16 block, give or take (a
    ratio near 1), and does not pass."""
    g, _ = load_golden(name)
    cfg, W, scales = _emulated(name, weight_files)
    import trunk_emulation as te
    xs = te.Trunk(cfg, W).trunk(planes=g["planes"][:4], scalars=g["scalars"][:4])
    for k in range(cfg.blocks):
        if cfg.block_kind(k) == "broadcast":
            continue
        x_in = xs[k].numpy()
        sk = bc.block_scales(cfg, scales, k)
        emu = bc.block(cfg, W, k, x_in, sk)
        fp16 = bc.block(cfg, W, k, x_in, None)
        near = bc.block(cfg, W, k, x_in, sk * np.float32(1 + 1e-6))
        off = bc.block(cfg, W, k, x_in, sk * np.float32(1 + 1e-3))
        ratio = lambda e: float(np.abs(e - emu).mean() / np.abs(e - fp16).mean())
        print(f"{name} block {k}: stand-in {ratio(near):.3f}, scales off by 1e-3 {ratio(off):.3f}")
        assert ratio(near) <= 0.25, (name, k, ratio(near))
        assert ratio(off) > 0.5, (name, k, ratio(off))


def _resources():
    """name -> (VGPRs, scratch bytes, LDS bytes, MFMAs, scratch instructions) of every k_block_i8 of geometry G128 (the
    mangled name carries the geometry struct) in the unit, from the kernel descriptors the build's compiler writes."""
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "block_i8.hip"), "-o", "-"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = r.stdout
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S*k_block_i8\S*G128\S*)\s*$", asm, re.M):
        name = m.group(1)
        desc = asm[m.start():asm.index(".end_amdhsa_kernel", m.start())]
        vg = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", desc).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1))
        start = re.search(r"^" + re.escape(name) + r":", asm, re.M).start()
        body = asm[start:asm.index(".Lfunc_end", start)]
        out[name] = (vg, scratch, lds, body.count("v_mfma_i32_16x16x64_i8"), "scratch_" in body)
    return out


def test_block_kernel_keeps_two_workgroups_per_cu_and_no_scratch():
    res = _resources()
    assert len(res) == 3, sorted(res)               # one, two and three inner layers
    for name, (vg, scratch, lds, mfma, uses_scratch) in res.items():
        assert scratch == 0 and not uses_scratch, name
        # two 256-thread workgroups per CU = two waves per SIMD: at most 256 VGPRs (arch + acc) a wave
        assert vg <= 256, (name, vg)
        # ... and half of the CU's 160 KiB of LDS each; the image is a static array, so this is all the kernel uses
        assert lds == 56448 and lds <= 81920, (name, lds)
        assert mfma > 0, name
    src = open(os.path.join(CSRC, "block_i8.hip")).read()
    # no dynamic LDS on top of the descriptor's: a geometry whose LDS fits a static array takes the static one in the
    # kernel and passes 0 dynamic bytes at launch, 256 threads a workgroup
    assert re.search(r"if constexpr \(kBytes <= kStaticLdsMax\) \{\s*__shared__ [^;]*\bsmem\[kBytes\];\s*return smem;", src)
    assert "constexpr int kDynLds = kLdsBytes <= kStaticLdsMax ? 0 : kLdsBytes;" in src
    assert re.search(r"dim3\(64 \* G::kWaves\), kDynLds, s, a\)", src)
    assert "constexpr int kStaticLdsMax = 64 * 1024;" in src
    assert re.search(r"struct G128 \{ static constexpr int C = 128, CB = 64, kWaves = 4, kWgPerCu = 2; \};", src)
    assert re.search(r"static_assert\(G::kWgPerCu \* kLdsBytes <= 160 \* 1024", src)   # two workgroups within the CU's LDS
