"""Writes tests/golden/nn_<name>.npz for the nets of netspec.WIDE_TRANSFORMER_CONFIGS: as make_transformer_golden.py does
for the d = 96 nets (wide_positions inputs, the same layout, the same attention criterion), from the float64
restatement of any width and head count, tests/tfm_restatement_dh.py, with 16 positions each.  Wq and Wk are scaled by
tfm_restatement_dh.QK_SCALES[name]; this script reports, per net, the smallest of 1.5, 2.0, 2.5, 3.0 that meets the
criterion, which that table must hold.

    python tests/golden/make_transformer_golden_dh.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_transformer_golden import MIN_PEAK, planes_and_scalars  # noqa: E402
from oracle.make_golden import wide_positions  # noqa: E402
from p3achygo_amd import netspec  # noqa: E402
import tfm_restatement_dh as dh  # noqa: E402

N_POS = 16


def dump(name, seed):
    pos = wide_positions(N_POS, seed)
    planes, sc = planes_and_scalars(pos)
    for scale in (1.5, 2.0, 2.5, 3.0):
        cfg, W = dh.fixture_weights(name, scale)
        probe = []
        ref = dh.forward(cfg, W, planes, sc, attn_probe=probe)
        peak = dh.attention_peak(probe)
        if (peak >= MIN_PEAK).all():
            break
    assert (peak >= MIN_PEAK).all(), f"attention too uniform: {peak}"
    assert scale == dh.QK_SCALES[name], f"{name}: QK_SCALES must hold {scale}"
    np.savez_compressed(
        os.path.join(HERE, f"nn_{name}.npz"),
        features=np.frombuffer(pos.tobytes(), np.uint8), n_pos=N_POS, planes=planes.astype(np.uint8), scalars=sc,
        raw=ref["raw"].astype(np.float32), move_probs=ref["move_probs"].astype(np.float32),
        value_probs=ref["value_probs"].astype(np.float32), score_probs=ref["score_probs"].astype(np.float32),
        opt_move_probs=ref["opt_move_probs"].astype(np.float32), attn_peak=peak, qk_scale=np.array(scale),
        weight_checksum=np.array([sum(float(w.astype(np.float64).sum()) for w in W.values()),
                                  sum(float((w.astype(np.float64) ** 2).sum()) for w in W.values())]))
    print(name, "qk scale", scale, "attention peak per head", np.round(peak, 3), flush=True)


if __name__ == "__main__":
    for i, name in enumerate(netspec.WIDE_TRANSFORMER_CONFIGS):
        dump(name, 71 + i)
