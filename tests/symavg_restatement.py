"""numpy restatement of symmetry-averaged evaluation (include/p3hip.h P3HIP_FLAG_SYMMETRY_AVG).

expand: the copies of every record, ordered by ascending symmetry, adjacent per slot, each as host/features.h
        FillFeatures would have built it under that symmetry.
reduce: the rows of a slot's copies, board-indexed entries rotated back (host/symmetry.h ApplyInverse), then
        acc = v_0; acc += v_1; ...; acc / k in float32.

A "row" is the engine's output row (csrc/kernels.h, kOutStride floats), put together from what the C ABI returns for
a slot: the result record (p3hip_get_slot) and the raw fields (p3hip_get_raw)."""
import numpy as np

GRIDS = ("board", "stones_atari", "stones_two_liberties", "stones_three_liberties", "stones_laddered")
OUT_STRIDE = 3416
BOARD_SEGMENTS = (0, 362, 1526, 1889, 3053)   # move logits, move probs, opt probs, opt logits, ownership
OWNERSHIP = slice(3053, 3414)


def syms_of(mask):
    return [s for s in range(8) if mask >> s & 1]


def expand(recs, mask, fwd):
    """n records -> n * k records, copy j of record r at r * k + j (fwd: the forward maps, [8][361])."""
    syms = syms_of(mask)
    k = len(syms)
    out = np.repeat(recs, k)
    lm = recs["last_moves"]
    li, lj = lm["i"].astype(np.int64), lm["j"].astype(np.int64)
    on = (li >= 0) & (li < 19) & (lj >= 0) & (lj < 19)
    for j, s in enumerate(syms):
        copy = out[j::k]
        m = fwd[s].astype(np.int64)
        for g in GRIDS:
            dst = np.empty_like(recs[g])
            dst[:, m] = recs[g]                      # out[fwd[s][i]] = in[i]
            copy[g] = dst
        t = m[np.where(on, li * 19 + lj, 0)]
        copy["last_moves"]["i"] = np.where(on, t // 19, li).astype(np.int32)
        copy["last_moves"]["j"] = np.where(on, t % 19, lj).astype(np.int32)
    return out


def row_of(result, raw):
    """the output row of one slot from its result record and its raw fields (include/p3hip.h p3hip_get_raw)"""
    r = np.zeros(OUT_STRIDE, np.float32)
    r[0:362] = np.ctypeslib.as_array(result.move_logits)
    r[362:724] = np.ctypeslib.as_array(result.move_probs)
    r[724:726] = np.ctypeslib.as_array(result.value_probs)
    r[726:1526] = np.ctypeslib.as_array(result.score_probs)
    r[1526:1888] = np.ctypeslib.as_array(result.opt_move_probs)
    r[1888] = result.err2_outcome
    r[1889:2251] = raw[362:724]       # opt logits
    r[2251:2253] = raw[724:726]       # outcome logits
    r[2253:3053] = raw[726:1526]      # score logits
    r[3053:3414] = raw[1526:1887]     # ownership
    r[3414] = raw[1888]               # gamma
    return r


def unrotate(row, s, fwd):
    """a copy's row under symmetry s back in the orientation of the slot: out[inv[s][i]] = in[i], i.e.
    out[p] = in[fwd[s][p]] on every board-indexed segment; everything else unchanged"""
    out = np.array(row, np.float32, copy=True)
    m = fwd[s].astype(np.int64)
    for b in BOARD_SEGMENTS:
        out[b:b + 361] = row[b + m]
    return out


def reduce(rows, mask, fwd):
    """k rows of one slot's copies (ascending symmetry) -> the averaged row"""
    syms = syms_of(mask)
    assert len(rows) == len(syms)
    acc = unrotate(rows[0], syms[0], fwd)
    for j in range(1, len(syms)):
        acc = acc + unrotate(rows[j], syms[j], fwd)   # float32 + float32, in order
    return acc / np.float32(len(syms))
