"""numpy restatement of the trainer's validation losses, written from the reference's Python with the lines cited; it
shares no code with the engine or p3achygo_amd/dataset.py.

    terms(raw, aux, tg)          the 19 per-position terms of include/p3hip.h from one position's raw outputs
                                 (p3hip_get_raw's layout), aux record (p3hip_get_aux's) and targets
                                 python/model.py:1297-1572 compute_losses + v1_loss_terms, per example;
                                 python/train.py:1139-1151 compute_accuracy
    batch_losses(T, coeffs)      the seventeen losses of one batch from its [n][19] terms: the means, the two batch-level
                                 clips and the weighted total (model.py:1359-1447, :1487-1516)
    val(batches, coeffs)         train.py val(): the per-batch losses averaged over batches (LossTracker.avg_losses),
                                 the hits over all positions (ValMetrics)
    parse_example / targets_from_example    a tf.Example by hand, and python/transforms.py _parse_example (:276-388) +
                                 _expand_common (:391-485) without the random symmetry and the last-move masking

dt = np.float64 is the checker.  dt = np.float32 is the "twin": the same formulas with every intermediate in float32 and
numpy's own summation order, which is how far a correct float32 evaluation (the trainer's is one) may lie from the exact
value; the GPU tests bound the kernel by four times that distance.

keras.metrics.kl_divergence(t, p): both clipped to [epsilon, 1] with epsilon = 1e-7 held in float32, then
sum t log(t / p).  keras.losses.Huber(): delta 1, error = y_pred - y_true."""
import struct

import numpy as np

RAW_LEN, AUX_LEN, NUM_TERMS = 1889, 837, 19
TERMS = ("policy", "policy_aux_dist", "policy_aux_scalar", "outcome", "q6", "q16", "q50", "score_pdf", "score_cdf", "own",
         "gamma_sq", "q_err", "q_score", "q_score_err", "pi_soft", "pi_optimistic", "mcts_dist", "move_hit", "outcome_hit")
LOSSES = ("loss", "policy", "policy_aux_dist", "policy_aux_scalar", "outcome", "q6", "q16", "q50", "score_pdf", "score_cdf",
          "own", "q_err", "q_score", "q_score_err", "pi_soft", "pi_optimistic", "mcts_dist")      # model.py:1428-1447
# python/loss_coeffs.py: the positional arguments of SLCoeffs() and RLCoeffs(), in the dataclass's field order
COEFF_FIELDS = ("w_pi", "w_pi_aux", "w_val", "w_outcome", "w_score", "w_own", "w_q6", "w_q16", "w_q50", "w_gamma", "w_q_err",
                "w_q_score", "w_q_score_err", "w_pi_soft", "w_pi_optimistic", "w_mcts_dist")
SL = dict(zip(COEFF_FIELDS, (1.0, 0.15, 1.0, 1.5, 0.02, 0, 0, 0, 0, 0.005, 0, 0, 0, 0, 0, 0.0)))
RL = dict(zip(COEFF_FIELDS, (1.0, 0.15, 1.0, 1.5, 0.02, 0.45, 0.7, 0.4, 0.3, 0.005, 3.0, 0.2, 0.2, 4.0, 1.0, 0.125)))

EPS32 = np.float32(1e-7)          # keras.backend.epsilon() in a float32 graph
ZEPS32 = np.float32(1e-6)         # model.py:1460


# ---- pieces ---------------------------------------------------------------------------------------
def softmax(x, dt):
    x = np.asarray(x).astype(dt)
    e = np.exp(x - x.max())
    return e / e.sum(dtype=dt)


def log_softmax(x, dt):
    x = np.asarray(x).astype(dt)
    s = x - x.max()
    return s - np.log(np.exp(s).sum(dtype=dt))


def kld(t, p, dt):
    t = np.clip(np.asarray(t).astype(dt), dt(EPS32), dt(1))
    p = np.clip(np.asarray(p).astype(dt), dt(EPS32), dt(1))
    return (t * np.log(t / p)).sum(dtype=dt)


def huber(y_true, y_pred, dt):
    e = dt(y_pred) - dt(y_true)
    a = abs(e)
    return dt(0.5) * e * e if a <= dt(1) else a - dt(0.5)


def score_index(margin) -> int:
    """transforms.py:244-251: floor, + 400, clamped to 0 .. 799."""
    k = int(np.floor(np.float32(margin))) + 400
    return min(max(k, 0), 799)


def optimistic_weight(q, q_pred, q_err, dt):
    """model.py:1531-1556; q, q_pred, q_err: the three horizons 6, 16, 50."""
    z = [(dt(q[h]) - dt(q_pred[h])) / np.sqrt(dt(q_err[h]) + dt(ZEPS32)) for h in range(3)]
    decay = 4.0 / 7.0
    zv = (dt(decay * 3) * z[0] + dt(decay * 1.5) * z[1] + dt(decay * 0.75) * z[2]) / dt(3)
    with np.errstate(over="ignore"):
        w = dt(1) / (dt(1) + np.exp(-((zv - dt(1)) * dt(3))))
    return min(max(w, dt(0)), dt(1))


def terms(raw, aux, tg, dt=np.float64) -> np.ndarray:
    """The 19 terms of one position.  raw: [1889] as p3hip_get_raw, aux: [837] as p3hip_get_aux, tg: one targets record
    (a numpy void of targets_dtype() or a dict with its fields)."""
    raw, aux = np.asarray(raw, np.float32), np.asarray(aux, np.float32)
    pi, opt, outcome, score = raw[0:362], raw[362:724], raw[724:726], raw[726:1526]
    own_pred, q6_err, gamma = raw[1526:1887], raw[1887], raw[1888]
    pi_aux, pi_soft = aux[0:362], aux[362:724]
    q_pred, q_err = aux[724:727], np.array([q6_err, aux[727], aux[728]], np.float32)
    qs_pred, qs_err, mcts_logits = aux[729:732], aux[732:735], aux[735:786]
    policy = np.asarray(tg["policy"], np.float32)
    margin = np.float32(tg["score_margin"])
    q = np.array([tg["q6"], tg["q16"], tg["q50"]], np.float32)
    qs = np.array([tg["q6_score"], tg["q16_score"], tg["q50_score"]], np.float32)
    has_dist, has_mcts = dt(int(tg["has_pi_aux_dist"]) != 0), dt(int(tg["has_mcts_value_dist"]) != 0)
    out = np.zeros(NUM_TERMS, dt)
    out[0] = kld(policy, softmax(pi, dt), dt)                                                  # :1304-1308
    out[1] = has_dist * kld(tg["policy_aux_dist"], softmax(pi_aux, dt), dt)                    # :1314-1322
    scce = -log_softmax(pi_aux, dt)[int(tg["policy_aux"])]                                     # :1325-1327
    out[2] = (dt(1) - has_dist) * min(max(scce, dt(0)), dt(50))
    g = (0.0, 1.0) if margin > 0 else (1.0, 0.0) if margin < 0 else (0.5, 0.5)                 # transforms.py:413-421
    out[3] = -(np.array(g, dt) * log_softmax(outcome, dt)).sum(dtype=dt)                       # :1330
    for h in range(3):
        out[4 + h] = (dt(q[h]) - dt(q_pred[h])) ** 2                                           # :1331-1333
    k = score_index(margin)
    out[7] = -log_softmax(score, dt)[k]                                                        # :1337-1339
    step = (np.arange(800) >= k).astype(dt)                                                    # cumsum of the one-hot
    out[8] = ((step - np.cumsum(softmax(score, dt), dtype=dt)) ** 2).sum(dtype=dt)             # :1340-1348
    out[9] = ((np.asarray(tg["own"]).astype(dt) - own_pred.astype(dt)) ** 2).mean(dtype=dt)    # :1351-1352
    out[10] = dt(gamma) * dt(gamma)                                                            # :1354-1357
    out[11] = sum(huber((dt(q_pred[h]) - dt(q[h])) ** 2, q_err[h], dt) for h in range(3)) / dt(3)           # :1465-1472
    out[12] = sum(huber(dt(qs[h]) / dt(10), dt(qs_pred[h]) / dt(10), dt) for h in range(3)) / dt(3)         # :1478-1486
    out[13] = sum(huber((dt(qs_pred[h]) - dt(qs[h])) ** 2 / dt(100), dt(qs_err[h]) / dt(100), dt) for h in range(3)) / dt(3)
    soft = np.power(policy.astype(dt), dt(0.25))                                               # :1518-1527
    with np.errstate(invalid="ignore", divide="ignore"):
        out[14] = kld(soft / soft.sum(dtype=dt), softmax(pi_soft, dt), dt)
    out[15] = kld(policy, softmax(opt, dt), dt) * optimistic_weight(q, q_pred, q_err, dt)      # :1531-1564
    counts = np.asarray(tg["mcts_value_dist"]).astype(dt)                                      # :1382-1393
    out[16] = has_mcts * kld(counts / max(counts.sum(dtype=dt), dt(1)), softmax(mcts_logits, dt), dt)
    out[17] = float(int(np.argmax(pi)) == int(np.argmax(policy)))                              # train.py:1140-1144
    out[18] = float((int(np.argmax(outcome)) == 1) == bool(margin >= 0))                       # train.py:1146-1150
    return out


def terms_rows(raw, aux, targets, dt=np.float64) -> np.ndarray:
    return np.stack([terms(raw[i], aux[i], targets[i], dt) for i in range(len(targets))])


def bounds(raw, aux, targets):
    """(want [n][19] float64, bound [n][19]): per term max(4 x the float32 twin's largest distance from float64 over these
    rows, 1e-6 max(1, |want|)); terms 17 and 18 are exact.  Also returns the twin's distance per term."""
    want = terms_rows(raw, aux, targets, np.float64)
    twin = terms_rows(raw, aux, targets, np.float32).astype(np.float64)
    dev = np.abs(twin - want).max(axis=0)
    bound = np.maximum(4.0 * dev[None, :], 1e-6 * np.maximum(1.0, np.abs(want)))
    bound[:, 17:] = 0.0
    return want, bound, dev


def check_against(got, want, bound, dev, label=""):
    """Asserts |got - want| <= bound everywhere; prints and returns, per term, the largest error over the twin's own
    distance (the ratio DESIGN.md section 14 tabulates) and over the bound."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - want)
    ratio = err.max(axis=0)[:17] / np.maximum(dev[:17], 1e-300)
    rel = (err / np.maximum(bound, 1e-300))[:, :17].max(axis=0)
    for j in range(17):
        print(f"{label} {TERMS[j]:18s} max|err| {err[:, j].max():.3e}  twin {dev[j]:.3e}  err/twin {ratio[j]:.3g}  err/bound {rel[j]:.3g}")
    assert np.isfinite(got).all(), "a term is not finite"
    bad = np.argwhere(err > bound)
    assert len(bad) == 0, [(int(i), TERMS[j], got[i, j], want[i, j], bound[i, j]) for i, j in bad[:8]]
    return ratio


# ---- one batch, and val() -------------------------------------------------------------------------
def batch_losses(T, c) -> dict:
    """compute_losses' return values (LOSSES) for one batch from its per-example terms T [n][19]."""
    m = np.asarray(T, np.float64).mean(axis=0)
    policy, aux_dist, aux_scalar, outcome, q6, q16, q50, pdf, cdf, own, gamma_sq = m[:11]
    q_err, pi_soft, pi_opt, mcts = m[11], m[14], m[15], m[16]
    q_score = float(np.clip(m[12], 0.0, 200.0))            # :1487-1489, the clip on the batch's value
    q_score_err = float(np.clip(m[13], 0.0, 1000.0))       # :1512-1516
    val_loss = c["w_val"] * (c["w_outcome"] * outcome + c["w_q6"] * q6 + c["w_q16"] * q16 + c["w_q50"] * q50 +
                             c["w_score"] * pdf + c["w_own"] * own) + c["w_score"] * cdf           # :1360-1378
    loss = (c["w_pi"] * policy + c["w_pi_aux"] * aux_dist + c["w_pi_aux"] * 0.6 * aux_scalar + val_loss +
            gamma_sq * c["w_gamma"] + c["w_mcts_dist"] * mcts)                                     # :1395-1402
    loss += (c["w_q_err"] * q_err + c["w_q_score"] * q_score + c["w_q_score_err"] * q_score_err +
             c["w_pi_soft"] * pi_soft + c["w_pi_optimistic"] * pi_opt)                             # :1420-1426
    vals = (loss, policy, aux_dist, aux_scalar, outcome, q6, q16, q50, pdf, cdf, own, q_err, q_score, q_score_err,
            pi_soft, pi_opt, mcts)
    return dict(zip(LOSSES, (float(v) for v in vals)))


def val(batches, c) -> dict:
    """batches: a list of [n_b][19] term arrays.  Losses: the mean over batches of batch_losses; accuracies: hits over
    all positions (train.py:1133-1154)."""
    per = [batch_losses(T, c) for T in batches]
    out = {k: float(np.mean([p[k] for p in per])) for k in LOSSES}
    n = sum(len(T) for T in batches)
    out["move_accuracy"] = float(sum(np.asarray(T)[:, 17].sum() for T in batches) / n)
    out["outcome_accuracy"] = float(sum(np.asarray(T)[:, 18].sum() for T in batches) / n)
    return out


# ---- a tf.Example by hand, and the record -> targets transform -------------------------------------
def _varint(b, i):
    v = shift = 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << shift
        shift += 7
        if not c & 0x80:
            return v, i


def _fields(b):
    """(field, wire, value) of every field of a message; value: int (wire 0), bytes (wire 1, 2, 5)."""
    i, out = 0, []
    while i < len(b):
        tag, i = _varint(b, i)
        field, wire = tag >> 3, tag & 7
        if wire == 0:
            v, i = _varint(b, i)
        elif wire == 1:
            v, i = b[i:i + 8], i + 8
        elif wire == 2:
            n, i = _varint(b, i)
            v, i = b[i:i + n], i + n
        elif wire == 5:
            v, i = b[i:i + 4], i + 4
        else:
            raise ValueError(f"wire type {wire}")
        out.append((field, wire, v))
    return out


def parse_example(payload: bytes) -> dict:
    """key -> (kind, values): kind 'bytes' (a list of bytes), 'float' (a list of float32) or 'int64'; a later map entry of
    the same key replaces an earlier one."""
    out = {}
    for f, w, features in _fields(payload):
        if (f, w) != (1, 2):
            continue
        for f2, w2, entry in _fields(features):
            if (f2, w2) != (1, 2):
                continue
            key = feature = None
            for f3, w3, v in _fields(entry):
                if (f3, w3) == (1, 2):
                    key = bytes(v).decode()
                elif (f3, w3) == (2, 2):
                    feature = v
            kind, values = None, []
            for f4, w4, lst in _fields(feature or b""):
                if w4 != 2 or f4 not in (1, 2, 3):
                    continue
                kind, values = {1: "bytes", 2: "float", 3: "int64"}[f4], []
                for f5, w5, v in _fields(lst):
                    if f5 != 1:
                        continue
                    if f4 == 1:
                        values.append(bytes(v))
                    elif f4 == 2 and w5 == 2:
                        values.extend(np.frombuffer(bytes(v), "<f4").tolist())
                    elif f4 == 2:
                        values.append(struct.unpack("<f", bytes(v))[0])
                    else:
                        values.append(v)
            out[key] = (kind, values)
    return out


FIXED_BYTES = {"own": 361, "pi": 362 * 4, "pi_aux": 2, "color": 1}
FIXED_FLOATS = ("score_margin", "q6", "q16", "q50", "q6_score", "q16_score", "q50_score")


def targets_from_example(ex: dict):
    """GroundTruth of one parsed record as a dict with p3hip_targets' fields, or None where
    tf.io.parse_single_example(EX_DESC) / decode_raw + reshape would fail (transforms.py:8-32, :282-333)."""
    for key, n in FIXED_BYTES.items():                       # FixedLenFeature([], tf.string) + reshape
        kind, v = ex.get(key, (None, []))
        if kind != "bytes" or len(v) != 1 or len(v[0]) != n:
            return None
    for key in FIXED_FLOATS:                                 # FixedLenFeature([], tf.float32)
        kind, v = ex.get(key, (None, []))
        if kind != "float" or len(v) != 1:
            return None
    opt = {}
    for key, n in (("pi_aux_dist", 362 * 4), ("mcts_value_dist", 51 * 4)):      # VarLenFeature(tf.string), :312-333
        kind, v = ex.get(key, (None, []))
        if kind is None or (kind == "bytes" and len(v) == 0):
            opt[key] = None
        elif kind == "bytes" and len(v[0]) == n:
            opt[key] = v[0]
        else:
            return None
    pi_aux = int(np.frombuffer(ex["pi_aux"][1][0], "<i2")[0])
    if not 0 <= pi_aux <= 361:                               # an index into 362 logits (model.py:1325)
        return None
    color = int(np.frombuffer(ex["color"][1][0], np.int8)[0])
    own = np.frombuffer(ex["own"][1][0], np.int8).astype(np.int32)
    own = own if color == 1 else -own                        # :452
    f = {k: np.float32(ex[k][1][0]) for k in FIXED_FLOATS}
    dist, mcts = opt["pi_aux_dist"], opt["mcts_value_dist"]
    return {
        "policy": np.frombuffer(ex["pi"][1][0], "<f4").copy(),
        "policy_aux_dist": np.frombuffer(dist, "<f4").copy() if dist is not None else np.zeros(362, np.float32),
        "own": own.astype(np.float32),
        "mcts_value_dist": (np.frombuffer(mcts, "<i4").astype(np.float32) if mcts is not None else np.zeros(51, np.float32)),
        "score_margin": f["score_margin"], "q6": f["q6"], "q16": f["q16"], "q50": f["q50"],
        "q6_score": f["q6_score"], "q16_score": f["q16_score"], "q50_score": f["q50_score"],
        "policy_aux": pi_aux, "has_pi_aux_dist": int(dist is not None), "has_mcts_value_dist": int(mcts is not None),
    }


def targets_of_payload(payload: bytes):
    """targets_from_example of a record; None as well where a Feature is malformed on the wire (no parse gets past that)."""
    try:
        return targets_from_example(parse_example(payload))
    except (ValueError, IndexError, struct.error):
        return None


def payloads(raw: bytes):
    """The payloads of a plain TFRecord stream."""
    off, out = 0, []
    while off < len(raw):
        n = struct.unpack_from("<Q", raw, off)[0]
        out.append(raw[off + 12:off + 12 + n])
        off += 16 + n
    return out


# ---- synthetic rows at trained-net magnitudes ------------------------------------------------------
def _peaked_logits(rng, top_index, top_prob=0.999, n=362, spread=14.0):
    """Logits whose softmax puts top_prob on one entry and spreads the rest over e^-spread .. 1 relative: entries on both
    sides of the 1e-7 clip."""
    x = -rng.random(n) * spread
    x[top_index] = -np.inf
    rest = np.exp(x).sum()
    x[top_index] = np.log(top_prob / (1.0 - top_prob) * rest)
    return x.astype(np.float32)


def synthetic(targets_dtype, n=8, seed=5):
    """(raw [n][1889], aux [n][837], targets [n]) built so that the first eight rows take every branch of k_loss_rows; the
    comments name what a row is there for.  Rows behind the eighth repeat the patterns on fresh random numbers."""
    rng = np.random.default_rng(seed)
    raw = np.zeros((n, RAW_LEN), np.float32)
    aux = np.zeros((n, AUX_LEN), np.float32)
    tg = np.zeros(n, targets_dtype)
    margins = (0.0, 0.5, -0.5, 1000.0, -1000.0, 3.5, -7.0, 12.25)
    has_dist = (1, 0, 1, 0, 1, 0, 0, 1)
    has_mcts = (1, 1, 0, 0, 1, 0, 1, 0)
    pol_aux = (0, 360, 361, 5, 0, 361, 360, 17)
    for i in range(n):
        p = i % 8
        top = int(rng.integers(0, 362))
        peaked = p % 2 == 0
        for lo, dst in ((0, raw), (362, raw), (0, aux), (362, aux)):     # pi, optimistic, aux, soft
            at = top if dst is raw and lo == 0 else int(rng.integers(0, 362))
            dst[i, lo:lo + 362] = _peaked_logits(rng, at) if peaked else rng.normal(0, 2, 362)
        if not peaked:                                                   # the prediction on `top`, clear of the runner-up
            raw[i, 0:362][top] = raw[i, 0:362].max() + np.float32(0.25)
        raw[i, 724:726] = rng.normal(0, 2, 2)
        if abs(raw[i, 724] - raw[i, 725]) < 1e-3:
            raw[i, 725] += np.float32(0.01)
        raw[i, 726:1526] = rng.uniform(-10, 10, 800)                     # score logits in +-10
        raw[i, 1526:1887] = np.float32(0.9999) * rng.choice([-1.0, 1.0], 361)     # saturated ownership
        raw[i, 1887] = rng.uniform(0.05, 4)                              # q6_err
        raw[i, 1888] = rng.normal(0, 1.5)                                # gamma
        aux[i, 724:727] = np.tanh(rng.normal(0, 1, 3))
        aux[i, 727:729] = rng.uniform(0.05, 4, 2)
        aux[i, 729:732] = rng.normal(0, 20, 3)
        aux[i, 732:735] = np.abs(rng.normal(0, 30, 3))
        aux[i, 735:786] = rng.normal(0, 3, 51)
        e = np.exp(aux[i, 735:786].astype(np.float64) - aux[i, 735:786].max())
        aux[i, 786:837] = e / e.sum()
        if p in (1, 5):                                                  # a one-hot policy: 361 entries at the clip
            tg["policy"][i][top if p == 1 else (top + 7) % 362] = 1
        else:                                                            # a policy peaked to 0.999, entries below 1e-7
            x = _peaked_logits(rng, top if p != 6 else (top + 11) % 362).astype(np.float64)
            e = np.exp(x - x.max())
            tg["policy"][i] = e / e.sum()
        e = np.exp(_peaked_logits(rng, int(rng.integers(0, 362)), 0.9).astype(np.float64))
        tg["policy_aux_dist"][i] = (e / e.sum()) * has_dist[p]
        tg["own"][i] = rng.choice([-1.0, 0.0, 1.0], 361)
        tg["mcts_value_dist"][i] = rng.integers(0, 40, 51) * has_mcts[p]
        tg["score_margin"][i] = margins[p]
        tg["q6"][i], tg["q16"][i], tg["q50"][i] = np.tanh(rng.normal(0, 1, 3))
        tg["q6_score"][i], tg["q16_score"][i], tg["q50_score"][i] = rng.normal(0, 20, 3)
        tg["policy_aux"][i], tg["has_pi_aux_dist"][i], tg["has_mcts_value_dist"][i] = pol_aux[p], has_dist[p], has_mcts[p]
        if p == 0:      # q errors of exactly 0 (the sqrt(eps) path), targets above the predictions: the weight saturates at 1;
            raw[i, 1887] = 0; aux[i, 727:729] = 0       # has_mcts with all counts zero: the total becomes 1
            aux[i, 724:727] = (0.1, -0.2, 0.3); tg["q6"][i], tg["q16"][i], tg["q50"][i] = 0.6, 0.3, 0.8
            tg["mcts_value_dist"][i] = 0
        elif p == 1:    # ... and below them: a weight under 1e-4; counts summing to 2^20
            raw[i, 1887] = 0; aux[i, 727:729] = 0
            aux[i, 724:727] = (0.1, -0.2, 0.3); tg["q6"][i], tg["q16"][i], tg["q50"][i] = -0.4, -0.7, -0.2
            tg["mcts_value_dist"][i] = rng.multinomial(1 << 20, np.full(51, 1 / 51))
        elif p == 2:    # q errors of 4 on exact predictions (a Huber residual of 4 in q_err); score residuals of 0.3 / 10
            raw[i, 1887] = 4; aux[i, 727:729] = 4
            tg["q6"][i], tg["q16"][i], tg["q50"][i] = aux[i, 724:727]
            aux[i, 729:732] = (10, -20, 5); tg["q6_score"][i], tg["q16_score"][i], tg["q50_score"][i] = 13, -23, 8
        elif p == 3:    # score residuals of 30 (300 points): the linear side of both score Hubers
            aux[i, 729:732] = (10, -20, 5); tg["q6_score"][i], tg["q16_score"][i], tg["q50_score"][i] = 310, -320, 305
        elif p == 4:    # an exact tie of the two largest logits: the lower index is the prediction, and the label's move
            a, b = sorted((top, (top + 150) % 362))
            raw[i, 0:362][[a, b]] = raw[i, 0:362].max() + np.float32(1)
            x = _peaked_logits(rng, a).astype(np.float64)
            e = np.exp(x - x.max())
            tg["policy"][i] = e / e.sum()
    return raw, aux, tg
