"""Calibrated INT8 of the layer-wise trunks, without a GPU: the quantizer's known answers, the quantized tensors of
each layer-wise config, the CPU emulation's own error against the float64 goldens (tests/int8_restatement.py), and the
compiled resources of the INT8 kernels (csrc/lconv_i8.hip)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden  # noqa: E402
import int8_restatement as ir  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")


def test_activation_quantizer_rounds_half_to_even_and_clamps():
    y = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49, 126.5, 127.4, 128.0, 1e9, -126.5, -127.6, -1e9], np.float32)
    want = [0, 2, 2, 0, -2, -2, 0, 126, 127, 127, 127, -126, -127, -127]
    assert ir.quantize(y, 1.0).tolist() == want
    assert ir.quantize(np.float32([1.0, 3.0, 5.0]), 2.0).tolist() == [0, 2, 2]   # 0.5, 1.5, 2.5
    assert ir.quantize(np.float32([3.0, -7.0]), 0.0).tolist() == [0, 0]        # an all-zero tensor's scale
    assert ir.quantize(np.float32(np.linspace(-300, 300, 1001)), 1.0).min() == -127   # -128 stays unused


def test_weight_quantizer_is_per_output_channel_and_symmetric():
    w = np.zeros((3, 3, 2, 3), np.float32)      # HWIO: [tap][tap][cin][cout]
    w[..., 0] = 0.01
    w[1, 1, 0, 0] = -2.54                        # channel 0: max |w| = 2.54 -> s_w = 0.02
    w[0, 0, 1, 1] = 127.0                        # channel 1: s_w = 1, values rint(w)
    w[0, 1, 0, 1] = 0.5
    w[0, 2, 0, 1] = 1.5
    sw = ir.weight_scales(w)
    q, sw2 = ir.quantize_weights(w)
    assert np.array_equal(sw, sw2) and sw.dtype == np.float32
    np.testing.assert_array_equal(sw, np.float32([2.54, 127.0, 0.0]) / np.float32(127))
    assert q[1, 1, 0, 0] == -127 and q[0, 0, 0, 0] == 0       # 0.01 / 0.02 = 0.5 -> 0 (half to even)
    assert q[0, 0, 1, 1] == 127 and q[0, 1, 0, 1] == 0 and q[0, 2, 0, 1] == 2
    assert not q[..., 2].any()                                   # an all-zero channel: scale 0, weights 0


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


@pytest.mark.parametrize("name", ir.LAYERWISE)
def test_quantized_tensors_of_each_layerwise_config(name):
    from p3achygo_amd import netspec
    cfg = netspec.CONFIGS[name]
    assert ir.is_layerwise(cfg)
    names = ir.quantized_tensors(cfg)
    per_block = {"btl": cfg.inner_layers + 2, "nbt": 6, "classic": 2}[cfg.block_type]
    n_blocks = sum(cfg.block_kind(i) != "broadcast" for i in range(cfg.blocks))
    assert len(names) == per_block * n_blocks
    assert [tuple(int(v) for v in re.findall(r"\d+", n)) for n in names] == _p3w_convs(cfg)
    # the emulation's calibration visits them in that order, one maximum each
    obs = []
    rng = np.random.default_rng(0)
    W = netspec.generate_weights(cfg, randomize=True)
    ir.forward(cfg, W, rng.integers(0, 2, (1, 19, 19, 15)).astype(np.float32), rng.normal(size=(1, 8)).astype(np.float32),
               observe=obs)
    assert len(obs) == len(names) and all(v > 0 for v in obs)


def test_no_quantized_tensors_outside_the_layerwise_trunks():
    from p3achygo_amd import netspec
    for name in ("b12c256btl3", "b12c128btl3", "test_b3c256nbt"):
        assert not ir.is_layerwise(netspec.CONFIGS[name]) and ir.quantized_tensors(netspec.CONFIGS[name]) == []


@pytest.mark.parametrize("name", sorted(ir.BOUNDS))
def test_emulation_error_is_within_half_the_gpu_bounds(built, weight_files, name):
    from oracle import oracle
    from p3achygo_amd import netspec
    g, _ = load_golden(name)
    cfg = netspec.CONFIGS[name]
    W = netspec.generate_weights(cfg, randomize=True)
    net = oracle.OracleNet(weight_files(name))
    scales = ir.minmax_scales(cfg, W, [net.fill_inputs(c) for c in ir.calibration_batches()])
    assert len(scales) == len(ir.quantized_tensors(cfg)) and (scales > 0).all()
    err = ir.errors(ir.forward(cfg, W, g["planes"], g["scalars"], scales=scales), g)
    for k, bound in ir.BOUNDS[name].items():
        assert err[k] <= 0.5 * bound, (name, k, err)
    # and the INT8 error is real: well above what the fp16 storage alone gives
    fp16 = ir.errors(ir.forward(cfg, W, g["planes"], g["scalars"]), g)
    assert err["logit"] > 4 * fp16["logit"]


def _resources():
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(CSRC, "lconv_i8.hip"), "-o", "-"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = r.stdout
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S*k_(?:lconv_i8|absmax)\S*)\s*$", asm, re.M):
        name = m.group(1)
        desc = asm[m.start():asm.index(".end_amdhsa_kernel", m.start())]
        vg = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", desc).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1))
        start = re.search(r"^" + re.escape(name) + r":", asm, re.M).start()
        body = asm[start:asm.index(".Lfunc_end", start)]
        out[name] = (vg, scratch, body.count("v_mfma_i32_16x16x64_i8"), "scratch_" in body)
    return out


def test_int8_kernels_keep_two_workgroups_per_cu_and_no_scratch():
    res = _resources()
    convs = {k: v for k, v in res.items() if "k_lconv_i8" in k}
    assert len(convs) == 10, sorted(res)             # the ten layer shapes and flag sets of launch_lconv
    assert any("k_absmax" in k for k in res)
    for name, (vg, scratch, mfma, uses_scratch) in res.items():
        assert scratch == 0 and not uses_scratch, name
        if "k_lconv_i8" in name:
            # 256-thread workgroups, two per CU = two waves per SIMD: at most 256 VGPRs (arch + acc) a wave
            assert vg <= 256, (name, vg)
            assert mfma > 0, name
