"""The head tests' fixture without a GPU (tests/heads_common.py): sharp_heads changes head tensors only and puts every
job of tests/test_heads_gpu.py into every regime named in heads_common.COVERAGE_MIN (asserted on the float64 reference
alone); the pinned bounds stand between 10 and 100 times what the float32 twin measures here; and mutants of the
restatement, each a slip a faster head kernel could make, exceed their segment's bound on the sharp fixture.

The gap this closes: under netspec.generate_weights(randomize=True) and trunk_emulation.HEADS_TOL, the fixture the head
kernels were tested on so far, mutants 1 (no clamp at 10), 3b (the > 20 branch of the softplus returning the wrong
term), 6 (a sigmoid that is inf / inf below -88.7) and 7 (a value softmax without max subtraction) change no output
beyond HEADS_TOL, because gamma (-0.8 .. 0.8), the q6_err logit (-0.9 .. 2.0) and the outcome logits (-0.9 .. 1.4)
stay near zero there; test_mutants asserts that they are missed there and caught here.

Two of the eight mutants first listed for this file behave otherwise than expected, and the test states what is true:
  * 3, the > 20 branch returning log1p(exp(20)), changes no output on any input: min(., 10) follows the branch, so
    every value of 10 or more that the branch returns is the same factor.  The branch of the kernels
    (`s > 20 ? s : log1pf(__expf(s))`) is therefore unobservable as long as it returns at least 10; even without it
    __expf overflows to inf and fminf(inf, 10) is 10.  The test asserts bit-equal outputs.  3b is a slip of that
    branch that can be seen: the stable form s + log1p(exp(-s)) without its s.
  * 5, tanh replaced by a clamp to +-1, is caught by the ordinary fixture as well: its ownership pre-activations have
    a median of 0.3 - 0.4 but reach 2.8 (the hand-made positions), where the clamp is 0.24 from tanh, 1200 times
    HEADS_TOL.  It is not among the mutants asserted missed there.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import heads_common as hc  # noqa: E402
import trunk_emulation as te  # noqa: E402

MUTANT_NET = "c256v64nbt"
MUTANTS = {1: ("no clamp at 10", "score"), 2: ("softplus replaced by max(gamma, 0)", "score"),
           3: ("the > 20 branch returns log1p(exp(20))", None),
           "3b": ("the > 20 branch returns log1p(exp(-s))", "score"), 4: ("the score grid shifted by one bin", "score"),
           5: ("ownership tanh replaced by a clamp to +-1", "ownership"),
           6: ("q6_err as 4 (1 - e / (1 + e)), e = exp(-s) in float32", "q6_err"),
           7: ("the value softmax without max subtraction in float32", "value_probs"),
           8: ("the pass logit without the -3", "pi")}
MISSED_BY_THE_ORDINARY_FIXTURE = (1, 3, "3b", 6, 7)


@pytest.fixture(scope="module")
def cases():
    """(net, fp32) -> what every test here needs of it, computed once: the sharp weights, x, the float64 reference with
    its stages, and the twin's raw"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    pos = hc.positions()
    out = {}
    for job in hc.JOBS:
        key = (job.net, job.fp32)
        if key in out:
            continue
        cfg, W0, W = hc.weights(job.net, pos)
        x = hc.trunk_x(cfg, W, pos, fp16=not job.fp32)
        want = hc.reference(cfg, W, x, job.fp32)
        out[key] = dict(cfg=cfg, W0=W0, W=W, x=x, want=want, st=hc.stages(x, hc.head_weights(W, job.fp32)),
                        twin=hc.twin_raw(cfg, W, x, job.fp32))
    return out


def test_jobs_reach_every_instantiation():
    """the six k_headsx and the four k_heads instantiations, k_heads behind P3HIP_NO_HFUSE, the any-width kernels, both
    fp32 plans, the three transformer streams and a hot trunk under each kernel"""
    fam = lambda f, env="": {(hc.config(j.net).channels, hc.config(j.net).c_val) for j in hc.JOBS
                             if j.family == f and j.env == env and not hc.is_tfm(hc.config(j.net)) and ":" not in j.net}
    assert fam("k_headsx") == {(c, v) for c in (128, 256) for v in (32, 48, 64)} == fam("k_heads", "P3HIP_NO_HFUSE")
    assert {(384, v) for v in (32, 48, 64, 80)} | {(192, 80), (64, 32), (512, 80), (96, 48)} == fam("k_heads")
    assert fam("fp32") == {(256, 64), (384, 80)}
    from p3achygo_amd import netspec
    for j in hc.JOBS:
        cfg = hc.config(j.net)
        assert cfg.blocks == 1
        if hc.is_tfm(cfg):
            assert netspec.transformer_supported(cfg.channels, cfg.bottleneck_channels)
        else:
            assert netspec.conv_supported(cfg), j.net
    tf = {(hc.config(j.net).channels, hc.stream_width(hc.config(j.net)), j.family) for j in hc.JOBS if hc.is_tfm(hc.config(j.net))}
    assert tf == {(96, 128, "fp32"), (96, 128, "k_headsx"), (192, 256, "k_headsx"), (384, 384, "k_heads")}
    assert len({j.name for j in hc.JOBS}) == len(hc.JOBS) and hc.BATCH % 4 and hc.BATCH % 2


def test_sharp_heads_changes_head_tensors_only(cases):
    allowed = {n + f for n in hc.MISH_INPUTS + ("value.gamma_out", "value.oq_out", "value.score_out") for f in (".w", ".b")}
    allowed |= {"value.own.w"}
    from p3achygo_amd import netspec
    allowed |= set(netspec.POLICY_OUT_TENSORS)
    for (net, _), c in cases.items():
        changed = {k for k in c["W"] if not np.array_equal(c["W"][k], c["W0"][k])}
        assert changed <= allowed and set(c["W"]) == set(c["W0"]), (net, changed - allowed)
        assert {n + ".w" for n in hc.MISH_INPUTS} | {"value.gamma_out.w", "value.own.w"} <= changed, net
        assert all(c["W"][k].dtype == np.float32 and c["W"][k].shape == c["W0"][k].shape for k in c["W"])


def test_stages_is_the_restatement(cases):
    """heads_common.stages, which the mutants and the regime counts come from, is tfm_restatement._heads"""
    for (net, fp32), c in cases.items():
        e = hc.worst(hc.segment_errors(c["st"]["raw"], c["want"]))
        assert max(e.values()) < 1e-12, (net, fp32, e)


def test_every_job_is_in_every_regime(cases):
    """the conditions of the issue, on the float64 reference alone; the hot trunks included"""
    for (net, fp32), c in cases.items():
        cov = hc.coverage(c["want"], hc.probs64(c["want"]), c["st"])
        print(net, "fp32" if fp32 else "fp16", cov)
        hc.assert_coverage(cov, net)
        assert "q6<-89" in cov and f"{hc.MISH_INPUTS[0]}<-20" in cov
    for net in hc.HOT:   # x in the hundreds
        assert float(cases[(net, False)]["x"].abs().max()) > 100


def test_the_raw_bounds_are_ten_times_the_twin(cases):
    tw = {k: (0.0, "") for k in hc.SEG_NAMES}
    for (net, fp32), c in cases.items():
        assert np.isfinite(c["twin"]).all(), net
        for k, v in hc.worst(hc.segment_errors(c["twin"], c["want"])).items():
            if v > tw[k][0]:
                tw[k] = (v, net + (":fp32" if fp32 else ""))
    for k, (v, net) in tw.items():
        print(f"twin {k}: {v:.3g} ({net}); bound {hc.BOUNDS[k]:.3g} = {hc.BOUNDS[k] / v:.1f} x")
    for k, (v, net) in tw.items():
        assert 10 * v <= hc.BOUNDS[k] <= 100 * v, (k, v, net, hc.BOUNDS[k])


def test_the_probability_bounds_are_ten_times_the_softmax_twin(cases):
    """softmax_twin on the float32-rounded reference logits of every job against the float64 softmax of the same"""
    tw = {k: (0.0, "") for k in hc.PROB_KEYS}
    for (net, fp32), c in cases.items():
        raw32 = c["want"].astype(np.float32)
        p64 = hc.probs64(raw32.astype(np.float64))
        for k, (a, b) in hc.PROB_SLICES.items():
            d = float(np.abs(hc.softmax_twin(raw32[:, a:b]) - p64[k]).max())
            if d > tw[k][0]:
                tw[k] = (d, net)
    for k, (v, net) in tw.items():
        print(f"softmax twin {k}: {v:.3g} ({net}); bound {hc.PROB_BOUNDS[k]:.3g} = {hc.PROB_BOUNDS[k] / v:.1f} x")
    for k, (v, net) in tw.items():
        assert 10 * v <= hc.PROB_BOUNDS[k] <= 100 * v, (k, v, net, hc.PROB_BOUNDS[k])


def _record(raw, no_max=False):
    raw32 = np.asarray(raw, np.float32)
    rec = {k: hc.softmax_twin(raw32[a:b], no_max and k == "value_probs").astype(np.float32)
           for k, (a, b) in hc.PROB_SLICES.items()}
    rec.update(move_logits=raw32[:362].copy(), err2_outcome=float(raw32[1887]))
    return rec


def _mutant_raw(c, W, m):
    return hc.stages(c["x"], hc.head_weights(W, False), mutant=m)["raw"]


def test_mutants(cases):
    """every mutant exceeds its segment's bound on the sharp fixture; which of them the ordinary fixture would have
    flagged (randomize=True weights on the same x, |raw| within HEADS_TOL; mutant 7: record_check on ordinary logits)"""
    c = cases[(MUTANT_NET, False)]
    ordinary = hc.reference(c["cfg"], c["W0"], c["x"])
    assert hc.check_raw("unmutated", c["st"]["raw"], c["want"]) and np.abs(ordinary).max() < 20
    missed = []
    for m, (what, seg) in MUTANTS.items():
        if m == 7:
            bad = 0
            for s in range(hc.BATCH):
                hc.record_check(c["want"][s], _record(c["want"][s]), f"slot {s}")
                try:
                    hc.record_check(c["want"][s], _record(c["want"][s], no_max=True), f"slot {s}")
                except AssertionError as exc:
                    bad += 1
                    assert "value_probs" in str(exc), exc
            assert bad >= 2, "mutant 7 passes record_check on the sharp fixture"
            flagged = False
            for s in range(hc.BATCH):
                try:
                    hc.record_check(ordinary[s], _record(ordinary[s], no_max=True))
                except AssertionError:
                    flagged = True
        elif seg is None:   # the clamp at 10 follows the branch: whatever it returns at or above 10 is the same output
            assert np.array_equal(_mutant_raw(c, c["W"], m), c["st"]["raw"]) and (c["want"][:, 1888] > 20).sum() >= 2
            print(f"mutant {m} ({what}): changes no output on any fixture")
            missed.append(m)
            continue
        else:
            with pytest.raises(AssertionError, match=f"segment {seg} ") as exc:
                hc.check_raw(f"mutant {m}", _mutant_raw(c, c["W"], m), c["want"])
            assert f"mutant {m}: segment {seg} " in str(exc.value)
            d = np.abs(_mutant_raw(c, c["W0"], m) - ordinary)
            flagged = not (d.max() <= te.HEADS_TOL)
        print(f"mutant {m} ({what}): caught on the sharp fixture; the ordinary fixture under HEADS_TOL would "
              f"{'' if flagged else 'NOT '}have flagged it")
        if not flagged:
            missed.append(m)
    assert set(MISSED_BY_THE_ORDINARY_FIXTURE) <= set(missed), missed


def test_check_raw_names_the_place_and_the_regime(cases):
    c = cases[(MUTANT_NET, False)]
    got = c["want"].copy()
    slot = int(np.argmax(c["want"][:, 1888] > 20))
    got[slot, 726 + 17] += 2 * hc.BOUNDS["score"] * np.abs(c["want"][slot, 726:1526]).max()
    with pytest.raises(AssertionError) as exc:
        hc.check_raw("job-name", got, c["want"], slots=list(range(100, 100 + hc.BATCH)))
    msg = str(exc.value)
    assert all(t in msg for t in ("job-name", "segment score", f"slot {100 + slot} ", "index 17", "got ", "want ", "gamma ",
                                  "softplus ", "clamped to 10", "past the branch at 20")), msg
    got = c["want"].copy()
    got[3, 1887] = np.nan
    with pytest.raises(AssertionError, match="segment q6_err"):
        hc.check_raw("job-name", got, c["want"])


def test_record_check_holds_the_record_to_the_raw_row(cases):
    c = cases[(MUTANT_NET, False)]
    raw = c["want"][int(np.argmax(hc.probs64(c["want"])["move_probs"].max(axis=1)))]
    hc.record_check(raw, _record(raw))
    for key, change in (("err2_outcome", lambda v: float(np.nextafter(np.float32(v), np.float32(9)))),
                        ("move_logits", lambda v: np.concatenate([v[:5], np.nextafter(v[5:6], np.float32(1e9)), v[6:]])),
                        ("score_probs", lambda v: v * np.float32(1 + 1e-3)),
                        ("opt_move_probs", lambda v: np.where(np.arange(362) == 7, np.float32("nan"), v))):
        rec = _record(raw)
        rec[key] = change(rec[key])
        with pytest.raises(AssertionError):
            hc.record_check(raw, rec, key)
