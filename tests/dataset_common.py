"""Shared by tests/test_dataset_cpu.py and tests/test_dataset_gpu.py: a TFRecord / tf.Example writer in plain Python
(to build records the recorder never writes), a wrapper of the host's recorder, and one scripted game."""
import ctypes as C
import glob
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "dataset", "mixed_schema.tfrecord")
FIXTURE_PAYLOADS = (4037, 4037, 4037, 5743, 5743, 5743)
NUM_MOVES, PASS = 362, 362       # moves: 1-based index, sign = colour (+ black)


# ---- TFRecord framing ----------------------------------------------------------------------------
def crc32c(data: bytes) -> int:
    table = crc32c.table
    crc = 0xFFFFFFFF
    for b in data:
        crc = table[(crc ^ b) & 0xFF] ^ (crc >> 8)
    return crc ^ 0xFFFFFFFF


crc32c.table = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0x82F63B78 if _c & 1 else _c >> 1
    crc32c.table.append(_c)


def masked_crc(data: bytes) -> int:
    crc = crc32c(data)
    return (((crc >> 15) | (crc << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def frame(payload: bytes) -> bytes:
    head = struct.pack("<Q", len(payload))
    return head + struct.pack("<I", masked_crc(head)) + payload + struct.pack("<I", masked_crc(payload))


def record_offsets(raw: bytes):
    """Offsets of the records of a plain TFRecord stream."""
    out, off = [], 0
    while off < len(raw):
        out.append(off)
        off += 16 + struct.unpack_from("<Q", raw, off)[0]
    return out


# ---- tf.Example by hand --------------------------------------------------------------------------
def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def ld(field: int, payload: bytes) -> bytes:
    return varint(field << 3 | 2) + varint(len(payload)) + payload


def bytes_feature(data: bytes) -> bytes:
    return ld(1, ld(1, data))


def float_feature(v: float, packed=True) -> bytes:
    f = struct.pack("<f", v)
    return ld(2, ld(1, f) if packed else varint(1 << 3 | 5) + f)


def example(features: dict, order=None, junk=False, tail=b"") -> bytes:
    """features: key -> encoded Feature.  order: the keys' order on the wire.  junk: unknown fields of every wire type
    in the Example, the Features and the map entries, and values in front of keys.  tail: more map entries behind."""
    fs = b""
    for k in (order or list(features)):
        key, val = ld(1, k.encode()), ld(2, features[k])
        entry = (varint(9 << 3 | 0) + varint(300) + val + key + varint(10 << 3 | 5) + b"abcd") if junk else key + val
        fs += ld(1, entry)
    fs += tail
    if junk:
        fs = varint(7 << 3 | 1) + b"12345678" + fs + ld(15, b"unknown")
        return ld(2, b"zz") + ld(1, fs) + varint(3 << 3 | 0) + varint(1 << 40)
    return ld(1, fs)


def base_features(color=1, margin=1.5, komi=7.5, last=(-20, -20, -20, 3, 361), hot=5) -> dict:
    grid = np.zeros(361, np.int8)
    board = grid.copy()
    board[3] = 1
    pi = np.zeros(NUM_MOVES, np.float32)
    pi[hot] = 1
    return {"bsize": bytes_feature(bytes([19])), "board": bytes_feature(board.tobytes()),
            "last_moves": bytes_feature(np.asarray(last, np.int16).tobytes()),
            "stones_atari": bytes_feature(grid.tobytes()), "stones_two_liberties": bytes_feature(grid.tobytes()),
            "stones_three_liberties": bytes_feature(board.tobytes()), "stones_in_ladder": bytes_feature(grid.tobytes()),
            "color": bytes_feature(np.int8(color).tobytes()), "pi": bytes_feature(pi.tobytes()),
            "score_margin": float_feature(margin), "komi": float_feature(komi)}


# ---- the host's recorder -------------------------------------------------------------------------
def recorder_lib():
    from p3achygo_amd import host_api
    lib = host_api.lib()
    lib.p3host_tfrec_new.restype = C.c_void_p
    lib.p3host_tfrec_new.argtypes = [C.c_char_p, C.c_int, C.c_char_p]
    lib.p3host_tfrec_free.argtypes = [C.c_void_p]
    lib.p3host_tfrec_flush.argtypes = [C.c_void_p]
    lib.p3host_tfrec_record.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float] + [C.c_void_p] * 7
    return lib


def loc(i, j, color):
    return color * (i * 19 + j + 1)


# a short game with a capture-free opening, a pass in the middle, komi 7.5; black starts
GAME = [loc(3, 3, 1), loc(15, 15, -1), loc(3, 15, 1), -PASS, loc(15, 3, 1), loc(9, 9, -1), loc(0, 0, 1), loc(18, 18, -1),
        loc(2, 9, 1), loc(16, 9, -1)]
KOMI = 7.5


def game_pi(n=len(GAME), seed=11) -> np.ndarray:
    rng = np.random.default_rng(seed)
    pi = rng.random((n, NUM_MOVES)).astype(np.float32) ** 8
    return (pi / pi.sum(axis=1, keepdims=True)).astype(np.float32)


def record_game(directory, games=1, moves=GAME, pi=None) -> str:
    """Records `games` copies of the scripted game through p3host_tfrec_record / flush; returns the chunk's path."""
    lib = recorder_lib()
    pi = game_pi(len(moves)) if pi is None else pi
    h = lib.p3host_tfrec_new(str(directory).encode(), 0, b"ds")
    mv = np.asarray(moves, np.int32)
    p = np.ascontiguousarray(pi, np.float32)
    for _ in range(games):
        assert lib.p3host_tfrec_record(h, mv.ctypes.data, len(mv), KOMI, p.ctypes.data, *([None] * 6)) == 0
    assert lib.p3host_tfrec_flush(h) == games * len(moves)
    lib.p3host_tfrec_free(h)
    (path,) = glob.glob(os.path.join(str(directory), "*.tfrecord.zz"))
    return path


def game_features(moves=GAME) -> np.ndarray:
    """p3host_game_features of the scripted game in front of every move, identity symmetry."""
    from p3achygo_amd import features, host_api
    L = host_api.lib()
    out = np.zeros(len(moves), features.features_dtype())
    g = L.p3host_game_new(KOMI)
    for m, mv in enumerate(moves):
        color = 1 if mv > 0 else -1
        L.p3host_game_features(g, color, 0, out.ctypes.data + m * out.dtype.itemsize)
        idx = abs(mv) - 1
        i, j = (19, 0) if idx == 361 else divmod(idx, 19)
        assert L.p3host_game_play(g, i, j, color)
    L.p3host_game_free(g)
    return out


# ---- synthetic output rows and labels for the scoring kernels -------------------------------------
def synthetic_rows(n_rows=96, seed=2):
    """Rows that hit every branch of k_score_rows; row i is pattern i % 18 over a seeded random base."""
    from p3achygo_amd import engine
    rng = np.random.default_rng(seed)
    mp = rng.random((n_rows, 362)).astype(np.float32) * np.float32(0.5) + np.float32(1e-3)
    vp = rng.random((n_rows, 2)).astype(np.float32) * np.float32(0.9) + np.float32(0.05)
    sp = rng.random((n_rows, 800)).astype(np.float32) * np.float32(0.5)
    lab = np.zeros(n_rows, engine.labels_dtype())
    lab["policy"] = rng.random((n_rows, 362)).astype(np.float32)
    lab["score_margin"] = (rng.integers(-80, 81, n_rows) + 0.5).astype(np.float32)
    lab["did_win"] = lab["score_margin"] >= 0
    one = np.float32(1.0)
    for i in range(n_rows):
        k = i % 18
        hot = int(rng.integers(0, 362))
        lab["policy"][i] = 0
        lab["policy"][i][hot] = 1
        if k == 0:      # the maxima at the first index and at the last score bin; a positive margin
            mp[i][0] = one; sp[i][799] = one; lab["score_margin"][i] = 12.5; lab["did_win"][i] = 1
        elif k == 1:    # the pass move 361 and score bin 0; a negative margin
            mp[i][361] = one; sp[i][0] = one; lab["score_margin"][i] = -30.5; lab["did_win"][i] = 0
        elif k == 2:    # a two-way tie, the label at the higher index: no hit
            mp[i][[100, 250]] = one; lab["policy"][i] = 0; lab["policy"][i][250] = 1
        elif k == 3:    # whole rows tied: index 0 everywhere
            mp[i] = np.float32(1 / 362); sp[i] = np.float32(1 / 800); vp[i] = 0.5
            lab["policy"][i] = np.float32(0.25)
        elif k == 4:    # ties across the lane-stride boundary (63 | 64 and 319 | 320): the lower index, another lane
            mp[i][[63, 64]] = one; sp[i][[319, 320]] = one
        elif k == 5:    # ... and the larger value right behind the boundary
            mp[i][63] = one; mp[i][64] = np.nextafter(one, np.float32(2)); sp[i][319] = one; sp[i][320] = np.nextafter(one, np.float32(2))
        elif k == 6:    # exact zeros where the losses look: both 16
            mp[i][hot] = 0; vp[i][int(lab["did_win"][i])] = 0
        elif k == 7:    # NaNs in the rows, not where the losses look
            mp[i][(hot + 5) % 362] = np.nan; sp[i][700] = np.nan; sp[i][[3, 650]] = one
        elif k == 8:    # margin -0.0 (a win), score bin 399 -> 0
            sp[i][399] = one; lab["score_margin"][i] = -0.0; lab["did_win"][i] = 1
        elif k == 9:    # score bin 400 -> 0 as well
            sp[i][400] = one; lab["score_margin"][i] = 0.5; lab["did_win"][i] = 1
        elif k == 10:   # the bins next to them: 398 -> -1 (i even) and 401 -> 1
            sp[i][398 if (i // 18) % 2 == 0 else 401] = one
        elif k == 11:   # a tie in the label: its lowest index; i odd: a label of zeros -> move 0
            lab["policy"][i] = 0
            if (i // 18) % 2 == 0:
                lab["policy"][i][[70, 200, 361]] = np.float32(1 / 3)
        elif k == 12:   # a NaN win probability never wins the argmax
            vp[i] = (0.25, np.nan); lab["did_win"][i] = 0; lab["score_margin"][i] = -1.5
        elif k == 13:   # an all-NaN score row: bin 0 -> -399
            sp[i] = np.nan
        elif k == 14:   # a denormal probability at the label's move
            mp[i][hot] = np.float32(3e-42)
        elif k == 15:   # -0.0 counts as zero: 16
            mp[i][hot] = np.float32(-0.0)
        elif k == 16:   # a tie between the last and the first index (lanes 41 and 0)
            mp[i][[0, 361]] = one; sp[i][[0, 799]] = one
        else:           # the loss of a probability of exactly 1 is 0; both value probabilities equal
            mp[i][hot] = one; vp[i] = 0.5
    return mp, vp, sp, lab
