"""The fused INT8 blocks at C = 128 / C_b = 64 (P3HIP_FLAG_INT8_C128, DESIGN.md section 9 "Fused INT8 blocks at
C = 128"): the served set, its fixtures and the bounds.

TEST INFRASTRUCTURE ONLY: used by tests/test_int8_c128_cpu.py and tests/test_int8_c128_gpu.py.  The emulation is that of
tests/int8_block_restatement.py, which takes the width from `cfg` (a block depends on the stored fp16 x alone); the
functions that ask whether a net is served are bound to this width here, everything else is re-exported as it is.
"""
from __future__ import annotations

import functools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import int8_block_restatement as br  # noqa: E402
from int8_block_restatement import _Q, block, block_scales, btl_block, calibration_batches, errors, fp16_weights  # noqa: E402,F401

WIDTHS = (128, 64)   # (C, C_b) of the trunks P3HIP_FLAG_INT8_C128 serves

# the trunks P3HIP_FLAG_INT8_C128 serves among the fixtures with a float64 golden
SERVED = ("test_b3c128btl2", "test_b5c128btl1_i2", "b12c128btl3")

# Bounds of the GPU tests against the float64 goldens (max |d| of move logits, move probabilities, value
# probabilities): three times the emulation's own error on the same fixture with its MinMax scales from
# calibration_batches(), rounded up, the larger of two measurements (the rule of int8_restatement.BOUNDS: where the
# quantizer rounds is fragile and the flips cascade).  The two measurements: the scales as calibrated, and the same
# scales times 1 + 1e-6, which moves the rounding boundaries as a difference of fp16 storage would.  The emulation's
# errors these come from (calibrated | times 1 + 1e-6):
#   test_b3c128btl2     0.0122 / 3.5e-5 / 1.36e-3  |  0.0120 / 3.5e-5 / 1.36e-3
#   test_b5c128btl1_i2  0.0272 / 1.1e-4 / 2.94e-3  |  0.0278 / 8.7e-5 / 2.52e-3
#   b12c128btl3         0.0373 / 1.6e-4 / 8.6e-4   |  0.0351 / 2.2e-4 / 1.88e-3
# (fp16 storage alone: 5.0e-4, 1.0e-3 and 2.7e-3 in the logits.)  tests/test_int8_c128_cpu.py checks that the emulation
# stays within half of each.
BOUNDS = {
    "test_b3c128btl2": {"logit": 0.04, "prob": 1.1e-4, "value_prob": 4.1e-3},
    "test_b5c128btl1_i2": {"logit": 0.085, "prob": 3.4e-4, "value_prob": 9e-3},
    "b12c128btl3": {"logit": 0.12, "prob": 6.7e-4, "value_prob": 5.7e-3},
}


is_served = functools.partial(br.is_served, widths=WIDTHS)
quantized_tensors = functools.partial(br.quantized_tensors, widths=WIDTHS)
forward = functools.partial(br.forward, widths=WIDTHS)
minmax_scales = functools.partial(br.minmax_scales, widths=WIDTHS)
