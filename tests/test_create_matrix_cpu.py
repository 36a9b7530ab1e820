"""What p3hip_create answers for every (net, precision flags) pair of a 16 x 10 matrix: accepted, or which refusal.

The refusals of csrc/plan.cpp choose_plan have an order of precedence (a `tiny` net with P3HIP_FLAG_FP32_TFM gets the
FP32_TFM message, not "unsupported architecture"; a C = 128 btl net with INT8 | INT8_FUSED gets INT8_FUSED's), and a
change to the plan's decision logic can swap two of them without any other test noticing.  The outcomes are compared
with tests/golden/create_matrix.json.

Record the golden file from the library of the commit whose behaviour is to be kept (P3HIP_LIB names it):
    P3HIP_LIB=/path/to/libp3hip.so python tests/test_create_matrix_cpu.py --record
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conftest import ROOT  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "create_matrix.json")

NETS = ["test_b3c128btl2", "test_b3c128nbt", "test_b3c256btl1", "test_b3c256nbt",
        "test_b3c384btl3", "test_b3c384nbt", "test_b3c192classic",
        "test_b5c256btl2_i2", "test_b3c64btl2", "test_b3c96nbt", "test_b3c128classic", "test_b4c512btl3_i2",
        "test_b2d96h3_tfm", "test_b2d64h2_tfm", "test_b2d384h6_tfm",
        "tiny"]
FLAG_SETS = ["0",
             "INT8", "INT8_FUSED", "INT8_C128",
             "FP32", "FP32_TFM", "FP32 | FP32_TFM",
             "INT8 | INT8_FUSED", "INT8_FUSED | INT8_C128", "FP32 | INT8"]


def _flags(names):
    from p3achygo_amd import engine
    return sum(getattr(engine, "FLAG_" + n.strip()) for n in names.split("|") if n.strip() != "0")


def outcome(path, flags):
    """'accepted' (created, or refused only for want of a device: the plan was built), or the refusal's first 60 characters"""
    from p3achygo_amd import engine
    try:
        engine.HipEngine(path, 4, flags=flags).close()
    except engine.EngineError as ex:
        text = str(ex)
        if "no HIP device" in text:
            return "accepted"
        return text[len("p3hip_create: "):][:60] if text.startswith("p3hip_create: ") else text[:60]
    return "accepted"


def matrix(directory):
    from p3achygo_amd import netspec
    out = {}
    for net in NETS:
        cfg = netspec.get_config(net)
        path = os.path.join(str(directory), net + ".p3w")
        netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
        out[net] = {fs: outcome(path, _flags(fs)) for fs in FLAG_SETS}
    return out


def test_every_create_outcome_is_the_recorded_one(built, tmp_path):
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(NETS) and all(sorted(want[n]) == sorted(FLAG_SETS) for n in NETS)
    got = matrix(tmp_path)
    wrong = [(n, fs, got[n][fs], want[n][fs]) for n in NETS for fs in FLAG_SETS if got[n][fs] != want[n][fs]]
    assert not wrong, wrong
    # the matrix tells the refusals apart: every kind of outcome occurs
    seen = {v for n in NETS for v in want[n].values()}
    for kind in ("accepted", "unsupported architecture", "INT8 is available only", "INT8 is not available for this conv trunk",
                 "INT8_FUSED is available only", "INT8_C128 is available only", "P3HIP_FLAG_FP32 serves",
                 "P3HIP_FLAG_FP32_TFM serves", "P3HIP_FLAG_FP32 cannot be combined"):
        assert any(v.startswith(kind) for v in seen), kind


if __name__ == "__main__" and "--record" in sys.argv:
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        json.dump(matrix(d), open(GOLDEN, "w"), indent=1, sort_keys=True)
        print("recorded", GOLDEN)
