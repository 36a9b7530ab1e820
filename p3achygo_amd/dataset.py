"""Recorded training chunks as labelled positions: read, score and calibrate.

    nn::GoDataset     cc/nn/engine/go_dataset.cc:32-123        -> Dataset, batches
    nn::Benchmark     cc/nn/engine/benchmark_engine.cc:77-108  -> score_chunks
    the calibrator's batches from a chunk (trt_calibrator.*)   -> calibrate_from_chunks
    train.py val()    python/train.py:1038-1160                -> loss_chunks, loss_from_sums, LossCoeffs

The chunk reader is host/tf_reader.h in libp3host.so; the scoring and the loss terms run on the device (csrc/score.hip,
csrc/loss.hip).
Unlike the reference a short last batch holds only the rows that were read (the reference scores the
default-constructed rows behind them), and a chunk with a bad record does not load at all.
"""
from __future__ import annotations

import dataclasses
from typing import Iterable, Iterator, Sequence, Tuple

import numpy as np

from . import host_api
from .engine import LOSS_TERMS, NUM_LOSS_TERMS, NUM_SCORE_TERMS, SCORE_TERMS, labels_dtype, targets_dtype
from .features import Result, features_dtype


class Dataset:
    """All rows of one chunk: `features` (features_dtype()), `labels` (labels_dtype()) and `targets` (targets_dtype())
    arrays of equal length.  has_targets[i]: the record holds every key the trainer's parse needs (python/transforms.py
    EX_DESC); where it does not, targets[i] is zeros and the row still scores.  Targets are as recorded: no symmetry."""

    def __init__(self, path: str, mode: int = host_api.DATASET_AUTO):
        h = host_api.dataset_open(path, mode)
        try:
            n = host_api.dataset_size(h)
            self.features = np.zeros(n, features_dtype())
            self.labels = np.zeros(n, labels_dtype())
            self.targets = np.zeros(n, targets_dtype())
            self.has_targets = np.zeros(n, bool)
            fs, ls, ts = self.features.dtype.itemsize, self.labels.dtype.itemsize, self.targets.dtype.itemsize
            for i in range(n):
                host_api.dataset_row(h, i, self.features.ctypes.data + i * fs, self.labels.ctypes.data + i * ls)
                self.has_targets[i] = host_api.dataset_targets(h, i, self.targets.ctypes.data + i * ts)
        finally:
            host_api.dataset_close(h)
        self.path = path

    def __len__(self) -> int:
        return len(self.features)


Chunk = Dataset


def batches(paths: Sequence[str], batch_size: int, max_batches: int | None = None, with_targets: bool = False) -> Iterator[Tuple[np.ndarray, ...]]:
    """(features, labels) batches of at most batch_size rows over the chunks in order, each chunk batched on its own
    as GoDataset does; the last batch of a chunk is short, never padded.  with_targets: (features, labels, targets,
    has_targets)."""
    done = 0
    for path in paths:
        ds = Dataset(path)
        for lo in range(0, len(ds), batch_size):
            if max_batches is not None and done >= max_batches:
                return
            hi = lo + batch_size
            if with_targets:
                yield ds.features[lo:hi], ds.labels[lo:hi], ds.targets[lo:hi], ds.has_targets[lo:hi]
            else:
                yield ds.features[lo:hi], ds.labels[lo:hi]
            done += 1


def release(engine, lo: int, hi: int) -> None:
    """Hands the results of slots lo .. hi - 1 over (p3hip_get_slot), so that later runs leave them out: a slot stays in
    every run until its result has been fetched or it is loaded again."""
    r = Result()
    for i in range(lo, hi):
        engine.GetBatch(i, r)


def load_batch(engine, feats: np.ndarray, labels: np.ndarray | None = None, prev_n: int = 0,
               targets: np.ndarray | None = None, has_targets: np.ndarray | None = None) -> int:
    """Rows into slots 0 .. len - 1, with their labels and their targets when given (has_targets: which rows have
    any; default all).  prev_n: rows of the batch loaded before; where this one is shorter, the slots behind it are
    released first, so that the run evaluates (and p3hip_score scores) only this batch.  Slots that are loaded again
    need no fetch.  Returns len(feats), the next call's prev_n."""
    n = len(feats)
    release(engine, n, prev_n)
    for i in range(n):
        engine.LoadBatch(i, feats[i:i + 1])
        if labels is not None:
            engine.load_labels(i, labels[i:i + 1])
        if targets is not None and (has_targets is None or has_targets[i]):
            engine.load_targets(i, targets[i:i + 1])
    return n


def stats_from_sums(sums: np.ndarray, n: int) -> dict:
    """The reference's DefaultStats (benchmark_engine.cc:45-75) from the sums of p3hip_score: running means there,
    sum / n here."""
    m = np.asarray(sums, np.float64) / max(n, 1)
    return {"num_examples": int(n), "policy_loss": m[0], "outcome_loss": m[1], "policy_percent": m[2],
            "outcome_percent": m[3], "score_diff": m[4], "score_pred_mean": m[5]}


def _argmax_rows(v: np.ndarray) -> np.ndarray:
    """Argmax of benchmark_engine.cc:11-22 per row: the lowest index among the largest non-NaN values above -FLT_MAX,
    0 when there is none."""
    with np.errstate(invalid="ignore"):
        ok = v > -np.finfo(np.float32).max
    return np.argmax(np.where(ok, v, -np.inf), axis=1)     # np.argmax: the first of equal maxima; a row of -inf: 0


def host_terms(move_probs, value_probs, score_probs, labels) -> np.ndarray:
    """The six terms of DefaultStats::Update per row on the host, [n][6] float64 (losses in float64 from the float32
    probability): what p3hip_score computes on the device, for the host-scoring leg of tools/dataset_benchmark.py."""
    n = len(labels)
    rows = np.arange(n)
    mv = _argmax_rows(labels["policy"])
    win = (labels["did_win"] != 0).astype(np.int64)
    pred = np.trunc(_argmax_rows(score_probs) + 0.5 - 400.0)      # `int score_pred = ...`: truncated toward zero

    def loss(p):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(p != 0, -np.log(p.astype(np.float64)), 16.0)

    diff = np.abs(labels["score_margin"].astype(np.float32) - pred.astype(np.float32))
    return np.stack([loss(move_probs[rows, mv]), loss(value_probs[rows, win]), (_argmax_rows(move_probs) == mv) * 1.0,
                     (_argmax_rows(value_probs) == win) * 1.0, diff.astype(np.float64), pred], axis=1)


def host_score(engine, labels: np.ndarray):
    """The host-scoring path: p3hip_get_slot for slots 0 .. len - 1 and host_terms on the results; (sums, n) like
    HipEngine.score()."""
    n = len(labels)
    mp, vp, sp = np.zeros((n, 362), np.float32), np.zeros((n, 2), np.float32), np.zeros((n, 800), np.float32)
    r = Result()
    for i in range(n):
        engine.GetBatch(i, r)
        mp[i], vp[i], sp[i] = r.move_probs, r.value_probs, r.score_probs
    return host_terms(mp, vp, sp, labels).sum(axis=0), n


def score_chunks(engine, paths: Iterable[str], max_batches: int | None = 1001) -> dict:
    """nn::Benchmark's loop without its warm-up and timing: per batch LoadBatch + labels, RunInference, p3hip_score.
    At most max_batches batches (the reference stops after 1001).  Returns stats_from_sums over everything scored."""
    total = np.zeros(NUM_SCORE_TERMS, np.float64)
    count = prev = 0
    for feats, labels in batches(list(paths), engine.batch_size, max_batches):
        prev = load_batch(engine, feats, labels, prev)
        engine.RunInference()
        sums, n = engine.score()
        total += sums
        count += n
    release(engine, 0, prev)
    return stats_from_sums(total, count)


def calibrate_from_chunks(engine, paths: Iterable[str], max_batches: int | None = None) -> int:
    """MinMax calibration of an INT8 engine (any of FLAG_INT8, FLAG_INT8_FUSED, FLAG_INT8_C128, FLAG_INT8_ANY, FLAG_INT8_CONV3) on the
    positions of recorded chunks: one p3hip_int8_calibrate per batch of engine.batch_size rows.  Returns the number of
    calibration batches."""
    nb = prev = 0
    for feats, _ in batches(list(paths), engine.batch_size, max_batches):
        prev = load_batch(engine, feats, None, prev)
        engine.int8_calibrate()
        nb += 1
    release(engine, 0, prev)
    if nb == 0:
        raise ValueError("calibrate_from_chunks: the chunks hold no positions")
    return nb


# ---- the trainer's validation losses (python/train.py val(), python/model.py compute_losses) -------------------------
@dataclasses.dataclass(frozen=True)
class LossCoeffs:
    """The weights of python/loss_coeffs.py as data: rl() is LossCoeffs.RLCoeffs(), sl() is SLCoeffs()."""
    w_pi: float
    w_pi_aux: float
    w_val: float
    w_outcome: float
    w_score: float
    w_own: float
    w_q6: float
    w_q16: float
    w_q50: float
    w_gamma: float
    w_q_err: float
    w_q_score: float
    w_q_score_err: float
    w_pi_soft: float
    w_pi_optimistic: float
    w_mcts_dist: float = 0.0

    @staticmethod
    def sl() -> "LossCoeffs":
        return LossCoeffs(1.0, 0.15, 1.0, 1.5, 0.02, 0.0, 0.0, 0.0, 0.0, 0.005, 0.0, 0.0, 0.0, 0.0, 0.0)

    @staticmethod
    def rl() -> "LossCoeffs":
        return LossCoeffs(1.0, 0.15, 1.0, 1.5, 0.02, 0.45, 0.7, 0.4, 0.3, 0.005, 3.0, 0.2, 0.2, 4.0, 1.0, 0.125)


LOSS_NAMES = ("loss",) + LOSS_TERMS[:10] + LOSS_TERMS[11:17]   # what compute_losses returns, in its order (:1428-1447)


def loss_from_sums(sums: np.ndarray, n: int, coeffs: LossCoeffs) -> dict:
    """The seventeen losses compute_losses returns for ONE batch (python/model.py:1297-1447, LOSS_NAMES) from the sums
    and count of p3hip_loss over that batch: the means, the two batch-level clips of v1_loss_terms (q_score to [0, 200],
    q_score_err to [0, 1000], :1487-1516) and the weighted total of :1359-1426 (0.6 on the scalar aux term, score_cdf
    outside w_val, w_gamma on the mean of gamma^2).  The total leaves out the L2 regulariser (model.losses, added by
    val_step): it needs the raw kernels, which a .p3w no longer holds.  float64 throughout."""
    m = dict(zip(LOSS_TERMS, np.asarray(sums, np.float64) / max(n, 1)))
    m["q_score"] = min(max(m["q_score"], 0.0), 200.0)
    m["q_score_err"] = min(max(m["q_score_err"], 0.0), 1000.0)
    c = coeffs
    val = c.w_val * (c.w_outcome * m["outcome"] + c.w_q6 * m["q6"] + c.w_q16 * m["q16"] + c.w_q50 * m["q50"] +
                     c.w_score * m["score_pdf"] + c.w_own * m["own"]) + c.w_score * m["score_cdf"]
    m["loss"] = (c.w_pi * m["policy"] + c.w_pi_aux * m["policy_aux_dist"] + c.w_pi_aux * 0.6 * m["policy_aux_scalar"] + val +
                 c.w_gamma * m["gamma_sq"] + c.w_mcts_dist * m["mcts_dist"] +
                 (c.w_q_err * m["q_err"] + c.w_q_score * m["q_score"] + c.w_q_score_err * m["q_score_err"] +
                  c.w_pi_soft * m["pi_soft"] + c.w_pi_optimistic * m["pi_optimistic"]))
    return {k: float(m[k]) for k in LOSS_NAMES}


def host_loss_terms(raw: np.ndarray, aux: np.ndarray, targets: np.ndarray) -> np.ndarray:
    """The 19 terms of p3hip_loss per row on the host, [n][19] float64, from fetched outputs: raw [n][RAW_LEN]
    (p3hip_get_raw), aux [n][AUX_LEN] (p3hip_get_aux), targets targets_dtype()[n].  The host leg of tools/gpu_loss_ab.py
    and the way to the numbers on an engine one cannot rebuild; include/p3hip.h has the definitions."""
    raw, aux = np.asarray(raw, np.float64), np.asarray(aux, np.float64)
    n = len(targets)
    eps = float(np.float32(1e-7))

    def lsm(x):
        s = x - x.max(axis=1, keepdims=True)
        return s - np.log(np.exp(s).sum(axis=1, keepdims=True))

    def kld(t, logits):
        t, p = np.clip(t, eps, 1.0), np.clip(np.exp(lsm(logits)), eps, 1.0)
        return (t * np.log(t / p)).sum(axis=1)

    def huber(y_true, y_pred):
        e = np.abs(y_pred - y_true)
        return np.where(e <= 1.0, 0.5 * e * e, e - 0.5)

    f = lambda name: targets[name].astype(np.float64)   # noqa: E731
    rows = np.arange(n)
    pi, opt, outcome, score = raw[:, 0:362], raw[:, 362:724], raw[:, 724:726], raw[:, 726:1526]
    pi_aux, pi_soft, mcts = aux[:, 0:362], aux[:, 362:724], aux[:, 735:786]
    q = np.stack([f("q6"), f("q16"), f("q50")], 1)
    qs = np.stack([f("q6_score"), f("q16_score"), f("q50_score")], 1)
    q_pred, qs_pred, qs_err = aux[:, 724:727], aux[:, 729:732], aux[:, 732:735]
    q_err = np.concatenate([raw[:, 1887:1888], aux[:, 727:729]], 1)
    policy, margin = f("policy"), f("score_margin")
    has_dist, has_mcts = (targets["has_pi_aux_dist"] != 0) * 1.0, (targets["has_mcts_value_dist"] != 0) * 1.0
    out = np.zeros((n, NUM_LOSS_TERMS), np.float64)
    out[:, 0] = kld(policy, pi)
    out[:, 1] = has_dist * kld(f("policy_aux_dist"), pi_aux)
    out[:, 2] = (1.0 - has_dist) * np.clip(-lsm(pi_aux)[rows, targets["policy_aux"]], 0.0, 50.0)
    g1 = np.where(margin > 0, 1.0, np.where(margin < 0, 0.0, 0.5))
    lo = lsm(outcome)
    out[:, 3] = -((1.0 - g1) * lo[:, 0] + g1 * lo[:, 1])
    out[:, 4:7] = (q - q_pred) ** 2
    k = np.clip(np.floor(margin) + 400.0, 0, 799).astype(np.int64)
    ls = lsm(score)
    out[:, 7] = -ls[rows, k]
    step = (np.arange(800)[None, :] >= k[:, None]) * 1.0
    out[:, 8] = ((step - np.cumsum(np.exp(ls), axis=1)) ** 2).sum(axis=1)
    out[:, 9] = ((f("own") - raw[:, 1526:1887]) ** 2).mean(axis=1)
    out[:, 10] = raw[:, 1888] ** 2
    out[:, 11] = huber((q_pred - q) ** 2, q_err).mean(axis=1)
    out[:, 12] = huber(qs / 10.0, qs_pred / 10.0).mean(axis=1)
    out[:, 13] = huber((qs_pred - qs) ** 2 / 100.0, qs_err / 100.0).mean(axis=1)
    soft = policy ** 0.25
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        out[:, 14] = kld(soft / soft.sum(axis=1, keepdims=True), pi_soft)
        z = ((q - q_pred) / np.sqrt(q_err + float(np.float32(1e-6)))) @ (np.array([3.0, 1.5, 0.75]) * (4.0 / 7.0)) / 3.0
        out[:, 15] = kld(policy, opt) * np.clip(1.0 / (1.0 + np.exp(-(z - 1.0) * 3.0)), 0.0, 1.0)
    counts = f("mcts_value_dist")
    out[:, 16] = has_mcts * kld(counts / np.maximum(counts.sum(axis=1, keepdims=True), 1.0), mcts)
    out[:, 17] = np.argmax(raw[:, 0:362], axis=1) == np.argmax(targets["policy"], axis=1)
    out[:, 18] = (np.argmax(outcome, axis=1) == 1) == (targets["score_margin"] >= 0)
    return out


def loss_chunks(engine, paths: Iterable[str], coeffs: LossCoeffs, max_batches: int | None = 10) -> dict:
    """train.py val() (python/train.py:1038-1160) on a FLAG_AUX engine: per batch of engine.batch_size rows LoadBatch +
    targets, RunInference, p3hip_loss and loss_from_sums; the per-batch losses averaged over the batches as
    LossTracker.avg_losses does (a short last batch weighs as much as a full one there too), the hits summed over all
    positions as ValMetrics does.  Rows whose record has no targets are evaluated and left out of the terms; a batch
    without any is skipped.  Positions are evaluated as recorded: the trainer's random symmetry and last-move masking
    (python/transforms.py:222, :424) are not mirrored.  Returns LOSS_NAMES, "move_accuracy", "outcome_accuracy",
    "batches" and "positions"."""
    acc = {k: 0.0 for k in LOSS_NAMES}
    nb = count = prev = 0
    hits = np.zeros(2, np.float64)
    for feats, _, targets, has in batches(list(paths), engine.batch_size, max_batches, with_targets=True):
        prev = load_batch(engine, feats, None, prev, targets, has)
        engine.RunInference()
        sums, n = engine.loss()
        if n == 0:
            continue
        for k, v in loss_from_sums(sums, n, coeffs).items():
            acc[k] += v
        hits += sums[17:19]
        nb += 1
        count += n
    release(engine, 0, prev)
    if nb == 0:
        raise ValueError("loss_chunks: the chunks hold no position with targets")
    out = {k: v / nb for k, v in acc.items()}
    out.update(move_accuracy=hits[0] / count, outcome_accuracy=hits[1] / count, batches=nb, positions=count)
    return out


__all__ = ["Dataset", "Chunk", "LossCoeffs", "LOSS_NAMES", "LOSS_TERMS", "loss_from_sums", "loss_chunks", "host_loss_terms", "batches", "load_batch", "release", "stats_from_sums", "host_terms", "host_score", "score_chunks",
           "calibrate_from_chunks", "SCORE_TERMS"]
