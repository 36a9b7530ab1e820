"""The fifteen aux outputs (P3HIP_FLAG_AUX, p3hip_get_aux) without a GPU: the ABI, the header's record layout and its
Python mirror against the ONNX names, the two refusals, the restatement of tests/aux_common.py tied to
heads_common.stages, the bounds held between 10 and 100 times what the float32 twin measures here, and mutants of the
restatement that each break their segment's bound on the sharp weights.

p3hip_cache_enable needs an engine, and an engine needs a device: what can be checked here is that the refusal stands in
front of the first device call of the function; tests/test_aux_outputs_gpu.py checks the refusal itself and its message.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import aux_common as ac  # noqa: E402
import heads_common as hc  # noqa: E402
from conftest import ROOT  # noqa: E402

MUTANT_NET = "c256v48btl"
MUTANTS = {"moves0": "pi_logits_aux", "soft_pass": "pi_logits_soft", "go_shift": "q", "no_abs": "q_score_err",
           "softmax_nomax": "mcts_dist_probs"}


@pytest.fixture(scope="module")
def cases():
    """job name -> x, the float64 reference, the stages and the twin's record, on the restatement's own trunk output"""
    pos = hc.positions()
    out = {}
    for job in ac.JOBS:
        cfg, W = ac.weights(job.net, pos)
        x = hc.trunk_x(cfg, W, pos, fp16=not job.fp32).numpy()
        st = ac.aux_stages(x, hc.head_weights(W, job.fp32))
        out[job.name] = dict(job=job, cfg=cfg, W=W, x=x, st=st, want=st["rec"], twin=ac.twin_rec(W, x, job.fp32))
    return out


def test_abi_header_and_mirror(built):
    from p3achygo_amd import engine
    import ctypes
    assert "p3hip_get_aux" in engine.EXPORTS
    assert ctypes.CDLL(engine.LIB_PATH).p3hip_get_aux   # AttributeError: the library does not export it
    header = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    assert re.search(r"^#define P3HIP_FLAG_AUX 1024u", header, re.M) and engine.FLAG_AUX == 1024
    flags = [int(v) for v in re.findall(r"^#define P3HIP_FLAG_\w+ (\d+)u", header, re.M)]
    assert flags.count(1024) == 1
    m = re.search(r"^#define P3HIP_AUX_LEN (\d+)", header, re.M)
    assert m and int(m.group(1)) == engine.AUX_LEN == ac.AUX_LEN == 837
    assert "int p3hip_get_aux(p3hip_engine* e, int slot, float out[P3HIP_AUX_LEN]);" in header
    # the header's layout table: every "[a..b]  NN:name ..." line against the mirror
    table = {}
    for a, b, names in re.findall(r"^ \*   \[(\d+)\.\.(\d+)\]\s+((?:\d\d:\w+ ?)+)", header, re.M):
        table[(int(a), int(b) + 1)] = names.split()
    assert len(table) == 8 and sum(len(v) for v in table.values()) == 15, table
    for (a, b), names in table.items():
        w = (b - a) // len(names)
        for k, n in enumerate(names):
            assert engine.AUX_SEGMENTS[n] == (a + k * w, a + (k + 1) * w), (n, a, b)
    # the kernel's offsets (csrc/heads_aux.h) are the header's
    src = open(os.path.join(ROOT, "p3achygo_amd", "csrc", "heads_aux.h")).read()
    offs = {k: int(v) for k, v in re.findall(r"constexpr int kAux(\w+) = (\d+);", src)}
    assert [offs[k] for k in ("OffPiAux", "OffPiSoft", "OffQ", "OffQErr", "OffQScore", "OffQScoreErr", "OffMctsLogits",
                              "OffMctsProbs", "Floats")] == [a for _, a, _ in ac.SEGMENTS] + [837]
    assert offs["Stride"] == 840 and offs["Stride"] % 4 == 0
    # the 25 names: the fixture, the mirror, one segment each, the aux record covered exactly once
    names = ac.output_names()
    assert len(names) == 25 and [int(n[:2]) for n in names] == list(range(25))
    assert list(engine.OUTPUT_NAMES) == names
    homes = [engine.AUX_SEGMENTS, engine.RAW_SEGMENTS, engine.RESULT_FIELDS]
    for n in names:
        assert sum(n in h for h in homes) == 1, n
    for segs, total in ((engine.AUX_SEGMENTS, engine.AUX_LEN), (engine.RAW_SEGMENTS, 1889)):
        cover = np.zeros(total, int)
        for a, b in segs.values():
            cover[a:b] += 1
        assert (cover == 1).all()
    rec = np.arange(837, dtype=np.float32)
    parts = engine.aux_outputs(rec)
    assert sorted(parts) == sorted(engine.AUX_SEGMENTS) and parts["24:mcts_dist_probs"][0] == 786 and len(parts["09:q6"]) == 1


def test_refusals_without_a_device(built, weight_files):
    from p3achygo_amd import engine
    L = engine.lib()
    for flags in (engine.FLAG_AUX | engine.FLAG_SYMMETRY_AVG, engine.FLAG_AUX | engine.FLAG_SYMMETRY_AVG | engine.FLAG_FP32):
        h = L.p3hip_create(weight_files("test_b3c256btl1").encode(), 4, 1, 0, flags)
        msg = (L.p3hip_create_error() or b"").decode()
        assert not h, "P3HIP_FLAG_AUX | P3HIP_FLAG_SYMMETRY_AVG was not refused"
        assert "P3HIP_FLAG_AUX cannot be combined with P3HIP_FLAG_SYMMETRY_AVG" in msg and "reference defines" in msg, msg
        assert "HIP device" not in msg
    # even for a file that does not exist: the refusal depends on the flags alone
    assert not L.p3hip_create(b"/nonexistent.p3w", 4, 1, 0, engine.FLAG_AUX | engine.FLAG_SYMMETRY_AVG)
    assert "P3HIP_FLAG_AUX cannot be combined" in L.p3hip_create_error().decode()
    # p3hip_cache_enable: the refusal comes before the function's first device call (bind)
    src = open(os.path.join(ROOT, "p3achygo_amd", "csrc", "engine.cpp")).read()
    body = src[src.index("int p3hip_cache_enable("):]
    body = body[:body.index("\n}\n")]
    assert 0 < body.index("P3HIP_FLAG_AUX") < body.index("not available on a P3HIP_FLAG_AUX engine") < body.index("e->bind()")
    assert body.index("e->bind()") < body.index("hipMalloc")


def test_aux_tensors_are_required_under_the_flag_only(built, tmp_path):
    """a file without value.mcts_dist fails p3hip_create with the usual list under the flag; without the flag it gets as far
    as the device"""
    from p3achygo_amd import engine, netspec
    cfg = netspec.CONFIGS["test_b3c256btl1"]
    W = netspec.generate_weights(cfg, randomize=True)
    path = str(tmp_path / "short.p3w")
    netspec.save_p3w(path, cfg, W)
    # rename the tensor in the file's table: same length, so every offset stays
    blob = open(path, "rb").read()
    assert blob.count(b"value.mcts_dist.w\0") == 1
    open(path, "wb").write(blob.replace(b"value.mcts_dist.w\0", b"value.mcts_dixt.w\0"))
    L = engine.lib()
    h = L.p3hip_create(path.encode(), 4, 1, 0, engine.FLAG_AUX)
    msg = L.p3hip_create_error().decode()
    assert not h and "lacks tensors" in msg and "value.mcts_dist.w" in msg, msg
    h = L.p3hip_create(path.encode(), 4, 1, 0, 0)
    msg = L.p3hip_create_error().decode()
    if h:
        L.p3hip_destroy(h)
    else:
        assert "lacks tensors" not in msg and "HIP device" in msg, msg


def test_restatement_is_heads_common_stages(cases):
    """what aux_stages shares with heads_common.stages equals it to 1e-12: go's columns 0, 1 and 5, the policy logits
    recomputed from its p and gp, gamma recomputed from its vp"""
    for name, c in cases.items():
        Wh = hc.head_weights(c["W"], c["job"].fp32)
        ref = hc.stages(c["x"], Wh)
        st = c["st"]
        T = lambda n: hc.tr._t(Wh[n], hc.F64)
        scale = max(1.0, np.abs(ref["go"]).max())
        assert np.abs(st["go"][:, [0, 1, 5]] - ref["go"][:, [0, 1, 5]]).max() <= 1e-12 * scale, name
        assert np.abs(st["go"] - ref["go"]).max() <= 1e-12 * scale, name
        p, gp, vp = (torch.from_numpy(st[k]) for k in ("p", "gp", "vp"))
        pi = torch.cat([hc.tr._conv(p, T("policy.out_moves.w")).reshape(len(p), 2, 361)[:, 0],
                        (hc.tr._dense(gp, Wh, "policy.out_pass", hc.F64) - 3)[:, 0:1]], dim=1).numpy()
        assert np.abs(pi - ref["raw"][:, :362]).max() <= 1e-12 * max(1.0, np.abs(pi).max()), name
        gamma = hc.tr._dense(hc.tr._mish(hc.tr._dense(vp, Wh, "value.gamma_pre", hc.F64)), Wh, "value.gamma_out", hc.F64).numpy()
        assert np.abs(gamma[:, 0] - ref["gamma"]).max() <= 1e-12 * max(1.0, np.abs(gamma).max()), name
        # sharp_aux left the outputs heads_common checks in their regimes
        want = ref["raw"]
        hc.assert_coverage(hc.coverage(want, hc.probs64(want), ref), name)


def test_sharp_weights_reach_the_regimes(cases):
    for name, c in cases.items():
        cov = ac.coverage(c["want"], c["st"])
        print(name, cov)
        ac.assert_coverage(cov, name)


def test_bounds_follow_the_twin(cases):
    """every constant of aux_common.BOUNDS and PROB_BOUND lies between 10 and 100 times the float32 twin's worst over the
    jobs, measured here; the twin itself passes check_rec on every job"""
    worst, where = dict.fromkeys(ac.SEG_NAMES, 0.0), {}
    prob, prob_where = 0.0, ""
    for name, c in cases.items():
        e = ac.worst(ac.segment_errors(c["twin"], c["want"]))
        for k, v in e.items():
            if v > worst[k]:
                worst[k], where[k] = v, name
        ref32 = c["want"][:, 735:786].astype(np.float32)
        d = float(np.abs(hc.softmax_twin(ref32) - hc.softmax64(ref32.astype(np.float64))).max())
        if d > prob:
            prob, prob_where = d, name
        ac.check_rec(name + " twin", c["twin"], c["want"])
    for k in ac.SEG_NAMES:
        print(f"{k}: twin {worst[k]:.3g} ({where.get(k)}), 15 x = {15 * worst[k]:.3g}, bound {ac.BOUNDS[k]:.3g}")
    print(f"softmax: twin {prob:.3g} ({prob_where}), 15 x = {15 * prob:.3g}, bound {ac.PROB_BOUND:.3g}")
    for k in ac.SEG_NAMES:
        assert 10 * worst[k] <= ac.BOUNDS[k] <= 100 * worst[k], (k, worst[k], ac.BOUNDS[k])
    assert 10 * prob <= ac.PROB_BOUND <= 100 * prob, (prob, ac.PROB_BOUND)


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_break_their_segment(cases, mutant):
    c = cases[MUTANT_NET]
    got = ac.aux_stages(c["x"], hc.head_weights(c["W"], False), mutant=mutant)["rec"]
    seg = MUTANTS[mutant]
    with pytest.raises(AssertionError) as exc:
        ac.check_rec(f"mutant {mutant}", got, c["want"])
    e = ac.segment_errors(got, c["want"])
    assert not e[seg].max() <= ac.BOUNDS[seg], (mutant, seg, e[seg].max())
    first = next(n for n in ac.SEG_NAMES if not e[n].max() <= ac.BOUNDS[n])
    assert f"segment {first} " in str(exc.value)
    print(f"mutant {mutant}: {seg} error {e[seg].max():.3g} over {ac.BOUNDS[seg]:.3g}")
