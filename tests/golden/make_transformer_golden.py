"""Writes tests/golden/nn_test_b2d96h3_tfm.npz and nn_b14d96h3_transformer.npz: wide_positions inputs and the
outputs of the float64 restatement tests/tfm_restatement.py (stored as float32, as the full-size conv fixtures are),
in the layout of the other nn_*.npz.  The weights are not stored: they are tfm_restatement.fixture_weights(name), the
seeded random init of netspec.TRANSFORMER_CONFIGS (randomize=True) with Wq and Wk scaled by QK_SCALE; their checksum
is stored.

Random-init q and k give a near-uniform attention (max probability ~1/361): a kernel with a wrong softmax or scale
would pass on it.  Wq and Wk are scaled until the mean over queries of the largest attention probability is at
least 0.05 (18x uniform) in every head of block 0, and that is asserted here.

    python tests/golden/make_transformer_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle.make_golden import wide_positions  # noqa: E402
from p3achygo_amd import netspec  # noqa: E402
import tfm_restatement as tfm  # noqa: E402

MIN_PEAK = 0.05


def planes_and_scalars(pos):
    """LoadPlanes / LoadFeatures of the fixture inputs (as oracle/make_golden.py states them)."""
    n = len(pos)
    planes = np.zeros((n, 19, 19, 15), np.float32)
    sc = np.zeros((n, 8), np.float32)
    for k in range(n):
        f = pos[k]
        col = int(f["color"])
        for ch, key in ((0, "board"), (7, "stones_atari"), (9, "stones_two_liberties"),
                        (11, "stones_three_liberties"), (13, "stones_laddered")):
            g = f[key].reshape(19, 19)
            planes[k, :, :, ch] = (g == col)
            planes[k, :, :, ch + 1] = (g == -col)
        for t in range(5):
            i, j = int(f["last_moves"][t]["i"]), int(f["last_moves"][t]["j"])
            if (i, j) == (19, 0):
                sc[k, 2 + t] = 1
            elif (i, j) != (-1, -1):
                planes[k, i, j, 2 + t] = 1
        sc[k, 0 if col == 1 else 1] = 1
        sc[k, 7] = (-1.0 if col == 1 else 1.0) * float(f["komi"]) / 15.0
    return planes, sc


def dump(name, n_pos, seed, store):
    cfg, W = tfm.fixture_weights(name)
    pos = wide_positions(n_pos, seed)
    planes, sc = planes_and_scalars(pos)
    probe = []
    ref = tfm.forward(cfg, W, planes, sc, attn_probe=probe)
    peak = probe[0].amax(-1).mean(dim=(0, 2)).numpy()        # per head: mean over positions and queries of max prob
    assert (peak >= MIN_PEAK).all(), f"attention too uniform: {peak}"
    np.savez_compressed(
        os.path.join(HERE, f"nn_{name}.npz"),
        features=np.frombuffer(pos.tobytes(), np.uint8), n_pos=n_pos, planes=planes.astype(np.uint8), scalars=sc,
        raw=ref["raw"].astype(store), move_probs=ref["move_probs"].astype(store),
        value_probs=ref["value_probs"].astype(store), score_probs=ref["score_probs"].astype(store),
        opt_move_probs=ref["opt_move_probs"].astype(store), attn_peak=peak, qk_scale=np.array(tfm.QK_SCALE),
        weight_checksum=np.array([sum(float(w.astype(np.float64).sum()) for w in W.values()),
                                  sum(float((w.astype(np.float64) ** 2).sum()) for w in W.values())]))
    print(name, "ok", ref["raw"].shape, "attention peak per head", peak, "max move prob", float(ref["move_probs"].max()))


if __name__ == "__main__":
    dump("test_b2d96h3_tfm", 64, 51, np.float32)
    dump("b14d96h3_transformer", 8, 52, np.float32)
