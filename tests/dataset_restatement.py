"""numpy restatement of the six per-position terms of DefaultStats::Update (cc/nn/engine/benchmark_engine.cc:25-61),
the reference for csrc/score.hip.  The losses are float64 -log of the float32 probability; everything else is exact.

    argmax        the sequential scan of :11-22: from (-FLT_MAX, index 0), advancing on strict >: the lowest index among
                  the largest non-NaN values above -FLT_MAX, index 0 when there is none
    policy_loss   -log(p), p = move_probs[argmax(labels.policy)]; 16 when p == 0
    outcome_loss  the same on value_probs[did_win]
    policy_hit    argmax(move_probs) == argmax(labels.policy)
    outcome_hit   argmax(value_probs) == did_win
    score_pred    int(argmax(score_probs) + 0.5 - 400), truncated toward zero (:30-31): 399 and 400 both give 0
    score_diff    |score_margin - float(score_pred)| in float32
"""
import numpy as np

TERMS = ("policy_loss", "outcome_loss", "policy_hit", "outcome_hit", "score_diff", "score_pred")
FLT_MAX = np.finfo(np.float32).max
MAX_LOSS = 16.0


def argmax_ref(v) -> int:
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        ok = v > -FLT_MAX            # False for NaN, -inf and -FLT_MAX itself
    if not ok.any():
        return 0
    m = v[ok].max()
    return int(np.flatnonzero(ok & (v == m))[0])


def argmax_scan(v) -> int:
    """The reference's loop, literally (slow; pins argmax_ref in the CPU test)."""
    best, arg = -FLT_MAX, 0
    for i, x in enumerate(np.asarray(v, np.float32)):
        if x > best:
            best, arg = x, i
    return arg


def ce_loss(p) -> float:
    p = np.float32(p)
    if p == 0:
        return MAX_LOSS
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(-np.log(np.float64(p)))


def score_pred_of(arg: int) -> int:
    return int(arg + 0.5 - 400)      # Python's int() truncates toward zero, as the C conversion does


def terms(move_probs, value_probs, score_probs, policy, score_margin, did_win) -> np.ndarray:
    """The six terms of one position as float64 (hits, score_diff and score_pred exactly what fp32 holds)."""
    mv = argmax_ref(policy)
    win = int(did_win != 0)
    pred = score_pred_of(argmax_ref(score_probs))
    diff = np.abs(np.float32(score_margin) - np.float32(pred))
    return np.array([ce_loss(np.asarray(move_probs, np.float32)[mv]), ce_loss(np.asarray(value_probs, np.float32)[win]),
                     float(argmax_ref(move_probs) == mv), float(argmax_ref(value_probs) == win), float(np.float32(diff)),
                     float(pred)], np.float64)


def terms_rows(move_probs, value_probs, score_probs, labels) -> np.ndarray:
    """[n][6] for rows [n][362], [n][2], [n][800] and n records of engine.labels_dtype()."""
    return np.stack([terms(move_probs[i], value_probs[i], score_probs[i], labels["policy"][i], labels["score_margin"][i],
                           labels["did_win"][i]) for i in range(len(labels))])


def ulp_distance(got, want) -> np.ndarray:
    """|got - want| in units of the fp32 spacing at |want| (want: float64); 0 where both are NaN or the same infinity."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        same = (np.isnan(got) & np.isnan(want)) | (got == want)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        d = np.abs(got - want) / ulp
    return np.where(same, 0.0, np.where(np.isfinite(d), d, np.inf))


def check_against(got_terms, want_terms, max_ulp=2.0):
    """Raises AssertionError unless hits, score_diff and score_pred are equal and both losses within max_ulp fp32 ulp of
    the float64 reference; returns the largest loss distance in ulp."""
    got = np.asarray(got_terms, np.float64).reshape(-1, 6)
    want = np.asarray(want_terms, np.float64).reshape(-1, 6)
    assert got.shape == want.shape, (got.shape, want.shape)
    for j in (2, 3, 4, 5):
        bad = np.flatnonzero(got[:, j] != want[:, j])
        assert bad.size == 0, (TERMS[j], bad[:8], got[bad[:8], j], want[bad[:8], j])
    d = ulp_distance(got[:, :2], want[:, :2])
    assert d.max() <= max_ulp, ("loss ulp distance", float(d.max()), np.argwhere(d > max_ulp)[:8])
    return float(d.max())
