"""Writes tests/golden/rope_spiral_d32_r4_b19.npz: the spiral RoPE cos / sin tables of the transformer trunk
(head_dim 32, 4 rotations, 19 x 19 board) as the reference itself computes them.

The reference module (python/model_transformer.py) imports TensorFlow at the top, so it is not imported: its
ROPE_THETA assignment and the spiral_rope_cos_sin_table function are picked out of the source with `ast` and
evaluated with numpy alone.  Only the resulting table is committed; tests compare the engine's own restatement of
it (p3hip_rope_table) with this file.

    python tests/golden/make_rope_fixture.py /path/to/reference/checkout
"""
import ast
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def reference_table(ref_root, num_rotations=4, head_dim=32, grid_len=19):
    path = os.path.join(ref_root, "python", "model_transformer.py")
    tree = ast.parse(open(path).read(), path)
    keep = [n for n in tree.body
            if (isinstance(n, ast.Assign) and any(getattr(t, "id", None) == "ROPE_THETA" for t in n.targets))
            or (isinstance(n, ast.FunctionDef) and n.name == "spiral_rope_cos_sin_table")]
    if len(keep) != 2:
        raise RuntimeError("ROPE_THETA / spiral_rope_cos_sin_table not found in " + path)
    ns = {"np": np, "math": math}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    cos, sin = ns["spiral_rope_cos_sin_table"](num_rotations, head_dim, grid_len)
    return float(ns["ROPE_THETA"]), np.asarray(cos, np.float64), np.asarray(sin, np.float64)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    theta, cos, sin = reference_table(sys.argv[1])
    assert cos.shape == sin.shape == (361, 32)
    np.savez_compressed(os.path.join(HERE, "rope_spiral_d32_r4_b19.npz"), cos=cos, sin=sin,
                        theta=np.array(theta), num_rotations=np.array(4), head_dim=np.array(32))
    print("rope table written, theta", theta)
