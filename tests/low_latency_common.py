"""What tests/test_low_latency_cpu.py and tests/test_low_latency_gpu.py share: the nets of the low-latency plan
(P3HIP_FLAG_LOW_LATENCY, csrc/conv_split.hip) under test, their files, and the tolerances.

The plan runs every conv trunk layer by layer with the rounding points of the runtime-width plan, so the nets of
netspec.WIDE_CONV_CONFIGS keep the table of tests/test_conv_widths_gpu.py.  The four nets whose default plan is the fused
block kernel have no layer-wise table yet: EMULATED below is the fp16 layer-wise emulation's error against the float64
restatement on them (cw.trunk(..., fp16=True), 16 positions, seed 11), as measured on the CPU and rounded up in the
third digit; tests/test_low_latency_cpu.py re-measures it.  Columns as in tests/test_conv_widths_gpu.py:
    test_b3c256btl1      1.19e-3 0.20  2.3e-6  6.6e-5  3.0e-7  3.8e-6  2.4e-8
    test_b3c128nbt       1.13e-3 0.19  4.8e-6  1.2e-4  2.6e-7  4.1e-6  3.5e-8
    test_b5c256btl2_i2   1.29e-3 0.21  2.7e-6  1.0e-4  3.8e-7  4.3e-6  4.5e-8
    test_b5c128btl1_i2   1.30e-3 0.22  3.1e-6  6.8e-5  1.4e-6  3.3e-6  4.7e-8
Every one stays below half of the bounds of tests/test_engine_gpu.py, so all four take those bounds.

TEST INFRASTRUCTURE ONLY."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import conv_widths_common as cw  # noqa: E402

FLAG = 4096   # engine.FLAG_LOW_LATENCY, include/p3hip.h P3HIP_FLAG_LOW_LATENCY
SPLITS = [(s, t) for s in (1, 2, 4) for t in (16, 32, 64)]   # the kernel's sets (csrc/conv_split.h)
# the default plan of these is the fused block kernel: the flag takes them layer by layer as well
FUSED_NETS = ["test_b3c256btl1", "test_b3c128nbt", "test_b5c256btl2_i2", "test_b5c128btl1_i2"]
WIDE_NETS = ["test_b3c64btl2", "test_b3c96nbt", "test_b3c192btl3", "test_b3c128classic", "test_b3c320nbt",
             "test_b4c512btl3_i2"]
BLOCK_NETS = ["test_b3c320nbt", "test_b4c512btl3_i2", "test_b3c128classic", "test_b5c256btl2_i2"]

_COLS = ("logit", "logit_share", "move_probs", "value_probs", "score_probs", "opt_move_probs", "kl")
EMULATED = {n: dict(zip(_COLS, v)) for n, v in {
    "test_b3c256btl1": (0.00119, 0.198, 2.31e-06, 6.62e-05, 3.01e-07, 3.79e-06, 2.4e-08),
    "test_b3c128nbt": (0.00113, 0.188, 4.83e-06, 0.000118, 2.62e-07, 4.15e-06, 3.47e-08),
    "test_b5c256btl2_i2": (0.00129, 0.215, 2.7e-06, 0.000104, 3.84e-07, 4.3e-06, 4.49e-08),
    "test_b5c128btl1_i2": (0.0013, 0.216, 3.13e-06, 6.76e-05, 1.42e-06, 3.3e-06, 4.71e-08),
}.items()}
# trunk_emulation.BOUNDS entries a net overrides because its twin exceeds half of them (tests/test_low_latency_cpu.py
# measures the twin on the four fused-default nets, the 37-position batch).  Worst error / lowest identical fraction:
# test_b3c256btl1 lw_btl 1.73 / 0.676, test_b3c128nbt lw_nbt 3.84 / 0.501, test_b5c256btl2_i2 lw_btl 0.98 / 0.876,
# test_b5c128btl1_i2 lw_btl 0.97 / 0.933, broadcast 0.88 / 0.885 at the worst, stem 0.80 / 1.000.  Only test_b3c256btl1's
# lw_btl passes half of its bound (3.0 / 2): it takes twice its twin's error, rounded up.  The three wide nets keep the
# bounds of tests/test_conv_widths_gpu.py.
BLOCK_BOUNDS = {n: {} for n in set(BLOCK_NETS) | set(FUSED_NETS)}
BLOCK_BOUNDS["test_b3c256btl1"] = {"lw_btl": (3.5, 0.62)}


def config(name):
    from p3achygo_amd import netspec
    return netspec.get_config(name)


def weights(name):
    from p3achygo_amd import netspec
    return netspec.generate_weights(config(name), randomize=True)


def tolerances():
    """name -> the six bounds of cw.check_outputs: the wide nets by the table of tests/test_conv_widths_gpu.py (same
    rounding points), the four fused-default nets by EMULATED, both through the rule of cw.tolerance"""
    from test_conv_widths_gpu import EMULATED as WIDE
    tol = {n: cw.tolerance(WIDE[n]) for n in WIDE_NETS}
    tol.update({n: cw.tolerance(EMULATED[n]) for n in FUSED_NETS})
    return tol
