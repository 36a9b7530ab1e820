"""Recorded training chunks as labelled positions: read, score and calibrate.

    nn::GoDataset     cc/nn/engine/go_dataset.cc:32-123        -> Dataset, batches
    nn::Benchmark     cc/nn/engine/benchmark_engine.cc:77-108  -> score_chunks
    the calibrator's batches from a chunk (trt_calibrator.*)   -> calibrate_from_chunks

The chunk reader is host/tf_reader.h in libp3host.so; the scoring runs on the device (csrc/score.hip).
Unlike the reference a short last batch holds only the rows that were read (the reference scores the
default-constructed rows behind them), and a chunk with a bad record does not load at all.
"""
from __future__ import annotations

from typing import Iterable, Iterator, Sequence, Tuple

import numpy as np

from . import host_api
from .engine import NUM_SCORE_TERMS, SCORE_TERMS, labels_dtype
from .features import Result, features_dtype


class Dataset:
    """All rows of one chunk: `features` (features_dtype()) and `labels` (labels_dtype()) arrays of equal length."""

    def __init__(self, path: str, mode: int = host_api.DATASET_AUTO):
        h = host_api.dataset_open(path, mode)
        try:
            n = host_api.dataset_size(h)
            self.features = np.zeros(n, features_dtype())
            self.labels = np.zeros(n, labels_dtype())
            fs, ls = self.features.dtype.itemsize, self.labels.dtype.itemsize
            for i in range(n):
                host_api.dataset_row(h, i, self.features.ctypes.data + i * fs, self.labels.ctypes.data + i * ls)
        finally:
            host_api.dataset_close(h)
        self.path = path

    def __len__(self) -> int:
        return len(self.features)


def batches(paths: Sequence[str], batch_size: int, max_batches: int | None = None) -> Iterator[Tuple[np.ndarray, np.ndarray]]:
    """(features, labels) batches of at most batch_size rows over the chunks in order, each chunk batched on its own
    as GoDataset does; the last batch of a chunk is short, never padded."""
    done = 0
    for path in paths:
        ds = Dataset(path)
        for lo in range(0, len(ds), batch_size):
            if max_batches is not None and done >= max_batches:
                return
            yield ds.features[lo:lo + batch_size], ds.labels[lo:lo + batch_size]
            done += 1


def release(engine, lo: int, hi: int) -> None:
    """Hands the results of slots lo .. hi - 1 over (p3hip_get_slot), so that later runs leave them out: a slot stays in
    every run until its result has been fetched or it is loaded again."""
    r = Result()
    for i in range(lo, hi):
        engine.GetBatch(i, r)


def load_batch(engine, feats: np.ndarray, labels: np.ndarray | None = None, prev_n: int = 0) -> int:
    """Rows into slots 0 .. len - 1, with their labels when given.  prev_n: rows of the batch loaded before; where this
    one is shorter, the slots behind it are released first, so that the run evaluates (and p3hip_score scores) only
    this batch.  Slots that are loaded again need no fetch.  Returns len(feats), the next call's prev_n."""
    n = len(feats)
    release(engine, n, prev_n)
    for i in range(n):
        engine.LoadBatch(i, feats[i:i + 1])
        if labels is not None:
            engine.load_labels(i, labels[i:i + 1])
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
    """MinMax calibration of an INT8 engine on the positions of recorded chunks: one p3hip_int8_calibrate per batch of
    engine.batch_size rows.  Returns the number of calibration batches."""
    nb = prev = 0
    for feats, _ in batches(list(paths), engine.batch_size, max_batches):
        prev = load_batch(engine, feats, None, prev)
        engine.int8_calibrate()
        nb += 1
    release(engine, 0, prev)
    if nb == 0:
        raise ValueError("calibrate_from_chunks: the chunks hold no positions")
    return nb


__all__ = ["Dataset", "batches", "load_batch", "release", "stats_from_sums", "host_terms", "host_score", "score_chunks",
           "calibrate_from_chunks", "SCORE_TERMS"]
