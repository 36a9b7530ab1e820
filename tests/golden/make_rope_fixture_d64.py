"""Writes tests/golden/rope_spiral_d64_r4_b19.npz: the spiral RoPE cos / sin tables of head width 64 (4 rotations,
19 x 19 board) as the reference itself computes them, extracted from its source exactly as make_rope_fixture.py does for
head width 32 (that script's reference_table).  Only the resulting table is committed; tests compare the engine's
p3hip_rope_table_dim(64) with it.

    python tests/golden/make_rope_fixture_d64.py /path/to/reference/checkout
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_rope_fixture import reference_table  # noqa: E402

if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    theta, cos, sin = reference_table(sys.argv[1], head_dim=64)
    assert cos.shape == sin.shape == (361, 64)
    np.savez_compressed(os.path.join(HERE, "rope_spiral_d64_r4_b19.npz"), cos=cos, sin=sin,
                        theta=np.array(theta), num_rotations=np.array(4), head_dim=np.array(64))
    print("rope table written, theta", theta)
