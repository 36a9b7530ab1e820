"""Python mirror of the reference's engine interface over the p3hip C ABI.

    nn::Engine            cc/nn/engine/engine.h:22-43      -> class HipEngine
    CreateEngine          cc/nn/engine/engine_factory.cc:56-73 -> create_engine
    KindFromEnginePath    cc/nn/engine/engine_factory.cc:16-35 -> kind_from_engine_path
    GetVersionFromModelPath  engine_factory.cc:37-53       -> get_version_from_model_path

Method names, argument meaning and failure behaviour follow the reference: the reference
aborts (CHECK / LOG(FATAL)) on engine failures, so every non-zero status of the C ABI is
raised as `EngineError` here.
"""
from __future__ import annotations

import ctypes as C
import enum
import os

import numpy as np

from .features import NUM_MOVES, RAW_LEN, Features, Result

_HERE = os.path.dirname(os.path.abspath(__file__))
# P3HIP_LIB lets tools/gpu_ab.py time two builds of the kernels side by side.
LIB_PATH = os.environ.get("P3HIP_LIB") or os.path.join(_HERE, "csrc", "libp3hip.so")

EXPORTS = [
    "p3hip_create", "p3hip_create_error", "p3hip_destroy", "p3hip_kind", "p3hip_path",
    "p3hip_batch_size", "p3hip_load_slot", "p3hip_run", "p3hip_get_slot", "p3hip_get_ownership",
    "p3hip_last_error", "p3hip_forward_resident", "p3hip_upload", "p3hip_sync", "p3hip_get_raw",
    "p3hip_time_trunk_kernel", "p3hip_flops_per_position", "p3hip_graph_state",
    "p3hip_cache_enable", "p3hip_load_slot_keyed", "p3hip_get_slot_keyed", "p3hip_cache_stats",
    "p3hip_blockw_stamps", "p3hip_debug_x", "p3hip_debug_tfm", "p3hip_rope_table", "p3hip_rope_table_dim",
    "p3hip_int8_calibrate", "p3hip_int8_scales", "p3hip_int8_set_scales",
    "p3hip_set_symmetries", "p3hip_symmetry_maps",
    "p3hip_create_rows", "p3hip_set_slot_symmetries", "p3hip_debug_symmetry_rows",
    "p3hip_load_labels", "p3hip_score", "p3hip_get_score", "p3hip_debug_score_rows",
    "p3hip_get_aux",
    "p3hip_load_targets", "p3hip_loss", "p3hip_get_loss", "p3hip_debug_loss_rows",
    "p3hip_debug_plan", "p3hip_debug_act_i8",
    "p3hip_debug_split", "p3hip_debug_pack_sconv", "p3hip_debug_tfm_split", "p3hip_debug_edge_split",
    "p3hip_debug_poison", "p3hip_debug_poison_table",
    "p3hip_debug_pack_wconv", "p3hip_debug_wconv_grid",
    "p3hip_graph_stats", "p3hip_debug_graph_table",
]

FLAG_RUN_ALL_SLOTS = 2
FLAG_SHARED_DEVICE = 4
FLAG_LAUNCH_GRAPH = 8
# a captured graph for runs of every size: a table of graphs keyed by slots, forward rows, feature buffer and result target;
# implies FLAG_LAUNCH_GRAPH (include/p3hip.h)
FLAG_LAUNCH_GRAPH_ANY = 131072
GRAPH_STATS = ("held", "captures", "replays", "launched", "evictions")
FLAG_INT8 = 16   # calibrated INT8 convs in the layer-wise blocks (include/p3hip.h)
FLAG_INT8_FUSED = 64   # calibrated INT8 of the C = 256 btl trunks, one fused int8 block kernel per block (section 9)
FLAG_INT8_C128 = 128   # the same for the C = 128 / C_b = 64 btl trunks (b12c128btl3): k_block_i8<128,64>, two workgroups per CU
FLAG_INT8_ANY = 2048   # calibrated INT8 whatever the conv trunk: the plan of one of the three flags above where one serves it,
# else layer by layer on k_lconv_i8_any at the padded widths (include/p3hip.h, DESIGN.md section 9 "INT8 at any width")
FLAG_INT8_CONV3 = 32768   # calibrated INT8 for the 3x3 convs of the layer-wise blocks only, every 1x1 conv in fp16 (include/p3hip.h,
# DESIGN.md section 9 "INT8 for the 3x3 convs only"); a classic trunk takes FLAG_INT8's / FLAG_INT8_ANY's plan
FLAG_WINOGRAD = 65536   # the 3x3 convs of the layer-wise blocks as F(2x2, 3x3) Winograd on fp16 MFMAs, everything else the fp16
# plan's own (include/p3hip.h); no calibration, its own parity bound
FLAG_FP32 = 256   # the conv trunks layer by layer in fp32, weights and activations included
FLAG_FP32_TFM = 512   # the transformer trunks in fp32, weights and activations included
FLAG_FP32_ANY = FLAG_FP32 | FLAG_FP32_TFM   # full precision whatever the trunk
NUM_SCORE_TERMS = 6
SCORE_TERMS = ("policy_loss", "outcome_loss", "policy_hit", "outcome_hit", "score_diff", "score_pred")
FLAG_AUX = 1024   # the model's other fifteen outputs on the device, one record per position
AUX_LEN = 837
# The 25 outputs of the network by their ONNX names (python/scripts/convert_to_onnx.py:462-488).  AUX_SEGMENTS: where the
# fifteen of the aux record lie (include/p3hip.h p3hip_get_aux); RAW_SEGMENTS: where p3hip_get_raw has seven of the other
# ten; the three distributions 01, 03 and 06 come from the result record (GetBatch).
AUX_SEGMENTS = {
    "08:pi_logits_aux": (0, 362), "21:pi_logits_soft": (362, 724),
    "09:q6": (724, 725), "10:q16": (725, 726), "11:q50": (726, 727),
    "13:q16_err": (727, 728), "14:q50_err": (728, 729),
    "15:q6_score": (729, 730), "16:q16_score": (730, 731), "17:q50_score": (731, 732),
    "18:q6_score_err": (732, 733), "19:q16_score_err": (733, 734), "20:q50_score_err": (734, 735),
    "23:mcts_dist_logits": (735, 786), "24:mcts_dist_probs": (786, 837),
}
RAW_SEGMENTS = {
    "00:pi_logits": (0, 362), "22:pi_logits_optimistic": (362, 724), "02:outcome_logits": (724, 726),
    "05:score_logits": (726, 1526), "04:own": (1526, 1887), "12:q6_err": (1887, 1888), "07:gamma": (1888, 1889),
}
RESULT_FIELDS = {"01:pi": "move_probs", "03:outcome": "value_probs", "06:score_probs": "score_probs"}
OUTPUT_NAMES = tuple(sorted(list(AUX_SEGMENTS) + list(RAW_SEGMENTS) + list(RESULT_FIELDS)))
# runs of 1 to about 64 positions: every conv trunk layer by layer through k_sconv, a position split across workgroups
# (include/p3hip.h)
FLAG_LOW_LATENCY = 4096
# the same for the transformer trunks: a block's launches split across more workgroups, the default fp16 plan's bits
# (include/p3hip.h)
FLAG_LOW_LATENCY_TFM = 8192
FLAG_LOW_LATENCY_ANY = FLAG_LOW_LATENCY | FLAG_LOW_LATENCY_TFM   # the low-latency plan whatever the trunk
FLAG_SYMMETRY_AVG = 32  # every slot averaged over a set of the eight symmetries on the device
# the same with a symmetry mask per slot, the copies of all slots packed densely (include/p3hip.h)
FLAG_SYMMETRY_SLOT = 16384


def labels_dtype() -> np.dtype:
    """numpy mirror of p3hip_labels (include/p3hip.h): the part of nn::GoLabels that DefaultStats reads."""
    return np.dtype([("policy", np.float32, (NUM_MOVES,)), ("score_margin", np.float32), ("did_win", np.int32)])


assert labels_dtype().itemsize == 4 * (NUM_MOVES + 2)

# The validation losses on the device (include/p3hip.h, "the trainer's validation losses"): the 19
# per-position terms of p3hip_loss in order.  The first seventeen are the per-example values of what
# P3achyGoModel.compute_losses + v1_loss_terms return (python/model.py:1297-1572), the last two train.py val()'s hits.
NUM_LOSS_TERMS = 19
LOSS_TERMS = ("policy", "policy_aux_dist", "policy_aux_scalar", "outcome", "q6", "q16", "q50", "score_pdf", "score_cdf",
              "own", "gamma_sq", "q_err", "q_score", "q_score_err", "pi_soft", "pi_optimistic", "mcts_dist", "move_hit",
              "outcome_hit")
NUM_V_BUCKETS = 51


def targets_dtype() -> np.dtype:
    """numpy mirror of p3hip_targets (include/p3hip.h): GroundTruth of python/transforms.py for one position."""
    f, i = np.float32, np.int32
    return np.dtype([("policy", f, (NUM_MOVES,)), ("policy_aux_dist", f, (NUM_MOVES,)), ("own", f, (361,)),
                     ("mcts_value_dist", f, (NUM_V_BUCKETS,)), ("score_margin", f), ("q6", f), ("q16", f), ("q50", f),
                     ("q6_score", f), ("q16_score", f), ("q50_score", f), ("policy_aux", i), ("has_pi_aux_dist", i),
                     ("has_mcts_value_dist", i)])


assert targets_dtype().itemsize == 4 * 1146 and len(LOSS_TERMS) == NUM_LOSS_TERMS


class EngineError(RuntimeError):
    pass


class Kind(enum.IntEnum):
    """Engine::Kind (engine.h:24-30) extended with kHip."""
    kUnknown = 0
    kTrt = 1
    kTF = 2
    kTFTrt = 3
    kTFXla = 4
    kHip = 5


_lib = None


def lib():
    """Loads libp3hip.so; fails loudly if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        L.p3hip_create.restype = C.c_void_p
        L.p3hip_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint32]
        L.p3hip_create_error.restype = C.c_char_p
        L.p3hip_destroy.argtypes = [C.c_void_p]
        L.p3hip_kind.argtypes = [C.c_void_p]
        L.p3hip_path.restype = C.c_char_p
        L.p3hip_path.argtypes = [C.c_void_p]
        L.p3hip_batch_size.argtypes = [C.c_void_p]
        L.p3hip_load_slot.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.p3hip_run.argtypes = [C.c_void_p]
        L.p3hip_get_slot.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.p3hip_get_ownership.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.p3hip_last_error.restype = C.c_char_p
        L.p3hip_last_error.argtypes = [C.c_void_p]
        L.p3hip_forward_resident.argtypes = [C.c_void_p, C.c_int]
        L.p3hip_upload.argtypes = [C.c_void_p]
        L.p3hip_sync.argtypes = [C.c_void_p]
        L.p3hip_get_raw.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.p3hip_cache_enable.argtypes = [C.c_void_p, C.c_int]
        L.p3hip_load_slot_keyed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int]
        L.p3hip_get_slot_keyed.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.p3hip_cache_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.p3hip_int8_calibrate.argtypes = [C.c_void_p]
        L.p3hip_int8_scales.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.p3hip_int8_set_scales.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.p3hip_set_symmetries.argtypes = [C.c_void_p, C.c_uint32]
        L.p3hip_symmetry_maps.argtypes = [C.c_void_p, C.c_void_p]
        L.p3hip_symmetry_maps.restype = None
        if hasattr(L, "p3hip_create_rows"):   # (P3HIP_LIB may name an earlier build of the library, tools/gpu_ab.py)
            L.p3hip_create_rows.restype = C.c_void_p
            L.p3hip_create_rows.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int]
            L.p3hip_set_slot_symmetries.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
            L.p3hip_debug_symmetry_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.p3hip_load_labels.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.p3hip_score.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.p3hip_get_score.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.p3hip_debug_score_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.POINTER(C.c_double)]
        L.p3hip_get_aux.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.p3hip_load_targets.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.p3hip_loss.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.p3hip_get_loss.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.p3hip_debug_loss_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                            C.POINTER(C.c_double)]
        L.p3hip_debug_plan.restype = C.c_char_p
        L.p3hip_debug_plan.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
        L.p3hip_time_trunk_kernel.restype = C.c_double
        L.p3hip_time_trunk_kernel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double),
                                              C.POINTER(C.c_char_p)]
        L.p3hip_flops_per_position.argtypes = [C.c_void_p, C.POINTER(C.c_double),
                                               C.POINTER(C.c_double)]
        _lib = L
    return _lib


def kind_from_engine_path(path: str) -> Kind:
    """engine_factory.cc:16-35 with the added rule `*.p3w` file -> kHip."""
    if os.path.isfile(path):
        ext = os.path.splitext(path)[1]
        if ext == ".p3w":
            return Kind.kHip
        if ext == ".trt":
            return Kind.kTrt
        if ext == ".pb":
            return Kind.kTFXla
        return Kind.kUnknown
    if os.path.basename(os.path.normpath(path)) == "_trt":
        return Kind.kTFTrt
    return Kind.kTF


def get_version_from_model_path(path: str) -> int:
    """engine_factory.cc:37-53: sibling VERSION file, default 1."""
    parent = os.path.dirname(path) if os.path.isfile(path) else path
    vf = os.path.join(parent, "VERSION")
    if os.path.isfile(vf):
        try:
            return int(open(vf).read().split()[0])
        except (ValueError, IndexError):
            pass
    return 1


class HipEngine:
    """nn::Engine over libp3hip.so (engine.h:22-43)."""

    def __init__(self, path: str, batch_size: int, version: int = 1, device: int = 0,
                 flags: int = 0, symmetry_rows: int = 0):
        """symmetry_rows: the forward rows a run of a FLAG_SYMMETRY_SLOT engine may evaluate (p3hip_create_rows);
        0 = 8 x batch_size."""
        self._L = lib()
        if symmetry_rows:
            self._h = self._L.p3hip_create_rows(path.encode(), batch_size, version, device, flags, symmetry_rows)
        else:
            self._h = self._L.p3hip_create(path.encode(), batch_size, version, device, flags)
        if not self._h:
            raise EngineError("p3hip_create: " + self._L.p3hip_create_error().decode())
        self.batch_size = batch_size

    # -- reference surface --------------------------------------------------------------
    def kind(self) -> Kind:
        return Kind(self._L.p3hip_kind(self._h))

    def path(self) -> str:
        return self._L.p3hip_path(self._h).decode()

    def LoadBatch(self, batch_id: int, features) -> None:
        ptr = features.ctypes.data if isinstance(features, np.ndarray) else C.addressof(features)
        self._ck(self._L.p3hip_load_slot(self._h, batch_id, ptr), "LoadBatch")

    def RunInference(self) -> None:
        self._ck(self._L.p3hip_run(self._h), "RunInference")

    def GetBatch(self, batch_id: int, result: Result = None) -> Result:
        result = result if result is not None else Result()
        self._ck(self._L.p3hip_get_slot(self._h, batch_id, C.addressof(result)), "GetBatch")
        return result

    def GetOwnership(self, batch_id: int) -> np.ndarray:
        own = np.zeros(361, np.float32)
        self._ck(self._L.p3hip_get_ownership(self._h, batch_id, own.ctypes.data), "GetOwnership")
        return own

    # -- on-device NN cache (include/p3hip.h) ---------------------------------------------
    def EnableCache(self, log2_entries: int) -> None:
        self._ck(self._L.p3hip_cache_enable(self._h, log2_entries), "EnableCache")

    def LoadBatchKeyed(self, batch_id: int, features, key_lo: int, key_hi: int, symmetry: int = 0) -> None:
        ptr = features.ctypes.data if isinstance(features, np.ndarray) else C.addressof(features)
        self._ck(self._L.p3hip_load_slot_keyed(self._h, batch_id, ptr, key_lo, key_hi, symmetry), "LoadBatchKeyed")

    def GetBatchKeyed(self, batch_id: int, result: Result = None):
        """(result, symmetry of the returned result, came from the table)"""
        result = result if result is not None else Result()
        sym, hit = C.c_int(0), C.c_int(0)
        self._ck(self._L.p3hip_get_slot_keyed(self._h, batch_id, C.addressof(result), C.byref(sym), C.byref(hit)), "GetBatchKeyed")
        return result, sym.value, bool(hit.value)

    def cache_stats(self) -> dict:
        out = (C.c_uint64 * 4)()
        self._L.p3hip_cache_stats(self._h, out)
        return {"lookups": out[0], "hits": out[1], "stored": out[2], "entries": out[3]}

    # -- calibrated INT8 (FLAG_INT8, FLAG_INT8_FUSED, FLAG_INT8_C128, FLAG_INT8_ANY) -----
    def int8_calibrate(self) -> None:
        """RunInference on the fp16 plan that also folds every quantized tensor's max |v| into the engine's running
        maxima (MinMax calibration): load a calibration batch, call this, fetch results as usual if wanted.  Any of
        FLAG_INT8, FLAG_INT8_FUSED and FLAG_INT8_C128."""
        self._ck(self._L.p3hip_int8_calibrate(self._h), "int8_calibrate")

    def int8_scales(self) -> np.ndarray:
        """The activation scales s_a = max / 127, block by block, conv by conv (the calibration cache); with
        FLAG_INT8_FUSED or FLAG_INT8_C128 (inner layers + 2) per btl block."""
        n = self._L.p3hip_int8_scales(self._h, None, 0)
        if n < 0:
            raise EngineError("int8_scales: the engine was not created with FLAG_INT8, FLAG_INT8_FUSED or FLAG_INT8_C128")
        out = np.zeros(n, np.float32)
        self._L.p3hip_int8_scales(self._h, out.ctypes.data, n)
        return out

    def set_int8_scales(self, scales) -> None:
        """Loads a saved calibration (what int8_scales returned by an engine of the same INT8 flag and net)."""
        s = np.ascontiguousarray(scales, np.float32)
        self._ck(self._L.p3hip_int8_set_scales(self._h, s.ctypes.data, len(s)), "set_int8_scales")

    # -- symmetry-averaged evaluation (FLAG_SYMMETRY_AVG) ----------------------------------
    def set_symmetries(self, mask: int) -> None:
        """Bit s selects symmetry s (identity, rot90, rot180, rot270, flip, flipRot90, flipRot180, flipRot270); 1..255.
        Applies from the next run.  Fails on an engine created without FLAG_SYMMETRY_AVG."""
        if not 0 <= int(mask) < 1 << 32:
            raise EngineError(f"set_symmetries: mask {mask} is not a uint32")
        self._ck(self._L.p3hip_set_symmetries(self._h, int(mask)), "set_symmetries")

    # -- a symmetry set per slot (FLAG_SYMMETRY_SLOT) -------------------------------------
    def set_slot_symmetries(self, batch_id: int, mask: int) -> None:
        """The symmetries (bit s = symmetry s, 1..255) of the position last loaded into the slot: after LoadBatch, before
        RunInference.  Every load resets the slot to 0x01.  Fails on an engine created without FLAG_SYMMETRY_SLOT."""
        if not 0 <= int(mask) < 1 << 32:
            raise EngineError(f"set_slot_symmetries: mask {mask} is not a uint32")
        self._ck(self._L.p3hip_set_slot_symmetries(self._h, batch_id, int(mask)), "set_slot_symmetries")

    # -- scoring against labels on the device (include/p3hip.h; DefaultStats, benchmark_engine.cc:25-61) ----
    def load_labels(self, batch_id: int, labels) -> None:
        """The labels (one labels_dtype() record, or its address) of the position last loaded into the slot; a new
        LoadBatch of the slot clears them."""
        ptr = labels.ctypes.data if isinstance(labels, np.ndarray) else labels
        self._ck(self._L.p3hip_load_labels(self._h, batch_id, ptr), "load_labels")

    def score(self):
        """Scores the rows of the last run whose slot has labels: (sums, n_scored), sums a float64 array in the order
        of SCORE_TERMS.  Fetches nothing."""
        sums = (C.c_double * NUM_SCORE_TERMS)()
        n = C.c_int(0)
        self._ck(self._L.p3hip_score(self._h, sums, C.byref(n)), "score")
        return np.array(sums[:], np.float64), n.value

    def get_score(self, batch_id: int):
        """The six terms of the slot from the last score(), or None when that call did not score the slot."""
        out = np.zeros(NUM_SCORE_TERMS, np.float32)
        rc = self._L.p3hip_get_score(self._h, batch_id, out.ctypes.data)
        if rc == 2:
            return None
        self._ck(rc, "get_score")
        return out

    def debug_score_rows(self, move_probs, value_probs, score_probs, labels):
        """Test hook: scores n synthetic rows ([n][362], [n][2], [n][800] floats) against labels (labels_dtype()[n]);
        returns (terms [n][6] float32, sums [6] float64).  Overwrites the last run's rows on the device."""
        mp = np.ascontiguousarray(move_probs, np.float32)
        vp = np.ascontiguousarray(value_probs, np.float32)
        sp = np.ascontiguousarray(score_probs, np.float32)
        lab = np.ascontiguousarray(labels, labels_dtype())
        n = len(lab)
        if mp.shape != (n, NUM_MOVES) or vp.shape != (n, 2) or sp.shape != (n, 800):
            raise EngineError("debug_score_rows: rows must be [n][362], [n][2] and [n][800] for n labels")
        terms = np.zeros((n, NUM_SCORE_TERMS), np.float32)
        sums = (C.c_double * NUM_SCORE_TERMS)()
        self._ck(self._L.p3hip_debug_score_rows(self._h, mp.ctypes.data, vp.ctypes.data, sp.ctypes.data, lab.ctypes.data,
                                                n, terms.ctypes.data, sums), "debug_score_rows")
        return terms, np.array(sums[:], np.float64)

    # -- the trainer's validation losses on the device (include/p3hip.h; python/model.py:1297-1572) ----
    def load_targets(self, batch_id: int, targets) -> None:
        """The targets (one targets_dtype() record, or its address) of the position last loaded into the slot; a new
        LoadBatch of the slot clears them.  Accepted on any engine."""
        ptr = targets.ctypes.data if isinstance(targets, np.ndarray) else targets
        self._ck(self._L.p3hip_load_targets(self._h, batch_id, ptr), "load_targets")

    def loss(self):
        """The loss terms of the rows of the last run whose slot has targets: (sums, n), sums a float64 array in the order
        of LOSS_TERMS (dataset.loss_from_sums turns them into the trainer's losses).  Needs FLAG_AUX.  Fetches nothing."""
        sums = (C.c_double * NUM_LOSS_TERMS)()
        n = C.c_int(0)
        self._ck(self._L.p3hip_loss(self._h, sums, C.byref(n)), "loss")
        return np.array(sums[:], np.float64), n.value

    def get_loss(self, batch_id: int):
        """The 19 terms of the slot from the last loss(), or None when that call did not handle the slot."""
        out = np.zeros(NUM_LOSS_TERMS, np.float32)
        rc = self._L.p3hip_get_loss(self._h, batch_id, out.ctypes.data)
        if rc == 2:
            return None
        self._ck(rc, "get_loss")
        return out

    def debug_loss_rows(self, raw, aux, targets):
        """Test hook: the terms of n synthetic rows (raw [n][RAW_LEN] in get_raw's layout, aux [n][AUX_LEN]) against
        targets (targets_dtype()[n]); returns (terms [n][19] float32, sums [19] float64).  Overwrites the last run's
        rows on the device."""
        rw = np.ascontiguousarray(raw, np.float32)
        ax = np.ascontiguousarray(aux, np.float32)
        tg = np.ascontiguousarray(targets, targets_dtype())
        n = len(tg)
        if rw.shape != (n, RAW_LEN) or ax.shape != (n, AUX_LEN):
            raise EngineError(f"debug_loss_rows: rows must be [n][{RAW_LEN}] and [n][{AUX_LEN}] for n targets")
        terms = np.zeros((n, NUM_LOSS_TERMS), np.float32)
        sums = (C.c_double * NUM_LOSS_TERMS)()
        self._ck(self._L.p3hip_debug_loss_rows(self._h, rw.ctypes.data, ax.ctypes.data, tg.ctypes.data, n,
                                               terms.ctypes.data, sums), "debug_loss_rows")
        return terms, np.array(sums[:], np.float64)

    # -- measurement / test hooks -------------------------------------------------------
    def load_all(self, feats_rec: np.ndarray) -> None:
        feats_rec = np.ascontiguousarray(feats_rec)
        sz = feats_rec.dtype.itemsize
        for i in range(len(feats_rec)):
            self._ck(self._L.p3hip_load_slot(self._h, i, feats_rec.ctypes.data + i * sz), "LoadBatch")

    def upload(self) -> None:
        self._ck(self._L.p3hip_upload(self._h), "upload")

    def forward_resident(self, n: int) -> None:
        self._ck(self._L.p3hip_forward_resident(self._h, n), "forward_resident")

    def sync(self) -> None:
        self._ck(self._L.p3hip_sync(self._h), "sync")

    def get_raw(self, batch_id: int) -> np.ndarray:
        raw = np.zeros(RAW_LEN, np.float32)
        self._ck(self._L.p3hip_get_raw(self._h, batch_id, raw.ctypes.data), "get_raw")
        return raw

    # -- the model's other fifteen outputs (FLAG_AUX) ----------------------------------------
    def GetAux(self, batch_id: int):
        """The aux record of the slot from the last run, AUX_LEN floats (aux_outputs splits it); None when the last run
        did not evaluate the slot.  Fails on an engine created without FLAG_AUX.  Fetches nothing."""
        out = np.zeros(AUX_LEN, np.float32)
        rc = self._L.p3hip_get_aux(self._h, batch_id, out.ctypes.data)
        if rc == 2:
            return None
        if rc != 0:
            raise EngineError(f"GetAux failed (rc={rc}): slot {batch_id} of {self.batch_size}, or the engine was created "
                              "without FLAG_AUX; " + self._L.p3hip_last_error(self._h).decode())
        return out

    def all_outputs(self, batch_id: int) -> dict:
        """All 25 outputs of the network for the slot, keyed by their ONNX names: seven from get_raw, fifteen from
        GetAux, the three distributions from GetBatch (which marks the slot fetched, so it is read last)."""
        raw, rec = self.get_raw(batch_id), self.GetAux(batch_id)
        if rec is None:
            raise EngineError(f"all_outputs: the last run did not evaluate slot {batch_id}")
        out = {k: raw[a:b].copy() for k, (a, b) in RAW_SEGMENTS.items()}
        out.update(aux_outputs(rec))
        res = self.GetBatch(batch_id)
        for k, f in RESULT_FIELDS.items():
            out[k] = np.ctypeslib.as_array(getattr(res, f)).copy()
        return {k: out[k] for k in OUTPUT_NAMES}

    def time_trunk_kernel(self, n_positions: int, iters: int):
        fl = C.c_double(0)
        name = C.c_char_p()
        ms = self._L.p3hip_time_trunk_kernel(self._h, n_positions, iters, C.byref(fl), C.byref(name))
        if ms < 0:
            raise EngineError("time_trunk_kernel: " + self._L.p3hip_last_error(self._h).decode())
        return ms, fl.value, (name.value or b"").decode()

    def debug_x(self, n: int, channels: int) -> np.ndarray:
        """residual stream after the last forward pass as [n][channels][361] floats"""
        out = np.zeros(n * channels * 361, np.float32)
        self._L.p3hip_debug_x.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self._ck(self._L.p3hip_debug_x(self._h, out.ctypes.data, n), "debug_x")
        return out.reshape(n, channels // 8, 361, 8).transpose(0, 1, 3, 2).reshape(n, channels, 361)

    def debug_tfm(self, which: int, n: int, heads: int, head_dim: int) -> np.ndarray:
        """what the last transformer block that ran left in device memory (p3hip.h p3hip_debug_tfm): which 0, 1, 2 = q,
        k, v as [n][heads][384][head_dim] floats, padding rows included; 3 = o as [n][361][heads * head_dim]"""
        shape = (n, heads, 384, head_dim) if which < 3 else (n, 361, heads * head_dim)
        out = np.zeros(shape, np.float32)
        self._L.p3hip_debug_tfm.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        self._ck(self._L.p3hip_debug_tfm(self._h, which, out.ctypes.data, n), "debug_tfm")
        return out

    def blockw_stamps(self) -> np.ndarray:
        """s_memtime stamps of k_blockw's _diag twin (P3HIP_BLOCKW=1 P3HIP_BLOCKW_DIAG=1): [wg 8][block 16][wave 4][24]"""
        out = np.zeros(8 * 16 * 4 * 24, np.uint64)
        self._L.p3hip_blockw_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        if self._L.p3hip_blockw_stamps(self._h, out.ctypes.data, out.size) != 0:
            raise EngineError("no k_blockw stamps (engine not created with P3HIP_BLOCKW_DIAG)")
        return out.reshape(8, 16, 4, 24)

    def debug_act_i8(self, n: int, channels: int) -> np.ndarray:
        """INT8 layer-wise engines: the int8 activated copy of x the last layer-wise block of the pass stored for the
        block behind it, as codes [n][channels][361] (channels: the padded C)"""
        out = np.zeros(n * channels * 361, np.int8)
        self._L.p3hip_debug_act_i8.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self._ck(self._L.p3hip_debug_act_i8(self._h, out.ctypes.data, n), "debug_act_i8")
        return out.reshape(n, channels // 16, 361, 16).transpose(0, 1, 3, 2).reshape(n, channels, 361)

    def debug_poison(self, byte: int) -> None:
        """Test hook (p3hip.h p3hip_debug_poison): fills every value buffer a forward pass must write before it reads it
        with `byte` (0..255); state, index records and the regions zeroed once stay.  The last run's results are gone."""
        self._L.p3hip_debug_poison.argtypes = [C.c_void_p, C.c_int]
        self._ck(self._L.p3hip_debug_poison(self._h, int(byte)), "debug_poison")

    def graph_state(self) -> int:
        """P3HIP_FLAG_LAUNCH_GRAPH: 1 replaying the captured forward pass, 0 not (yet), -1 capture failed."""
        self._L.p3hip_graph_state.argtypes = [C.c_void_p]
        return int(self._L.p3hip_graph_state(self._h))

    def graph_stats(self) -> dict:
        """p3hip_graph_stats: the graphs held now, and since the engine was created the captures, the replays, the forward
        passes launched kernel by kernel and the evictions (GRAPH_STATS).  FLAG_LAUNCH_GRAPH_ANY: of the engine's table;
        FLAG_LAUNCH_GRAPH alone: of its one graph.  EngineError on an engine with neither flag."""
        self._L.p3hip_graph_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        out = (C.c_uint64 * 5)()
        if self._L.p3hip_graph_stats(self._h, out) != 0:
            raise EngineError("graph_stats: the engine was created without FLAG_LAUNCH_GRAPH or FLAG_LAUNCH_GRAPH_ANY")
        return dict(zip(GRAPH_STATS, (int(v) for v in out)))

    def flops_per_position(self):
        t, c = C.c_double(0), C.c_double(0)
        self._L.p3hip_flops_per_position(self._h, C.byref(t), C.byref(c))
        return t.value, c.value

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.p3hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc: int, what: str) -> None:
        if rc != 0:
            raise EngineError(f"{what} failed (rc={rc}): " + self._L.p3hip_last_error(self._h).decode())


def aux_outputs(rec) -> dict:
    """Splits an aux record (GetAux) into its fifteen outputs, keyed by their ONNX names."""
    rec = np.asarray(rec)
    if rec.shape[-1] != AUX_LEN:
        raise ValueError(f"an aux record has {AUX_LEN} floats, not {rec.shape[-1]}")
    return {k: rec[..., a:b] for k, (a, b) in AUX_SEGMENTS.items()}


def debug_plan(path: str, flags: int = 0):
    """(trunk path name, quantized tensors, digest of the int8 weights and weight scales) of the host-side plan that
    p3hip_create would build for (file, flags, the P3HIP_* environment): p3hip_debug_plan, no device needed.  Raises
    EngineError with p3hip_create's reason where that returns NULL."""
    L = lib()
    n_q, dig = C.c_int(0), C.c_uint64(0)
    name = L.p3hip_debug_plan(path.encode(), flags, C.byref(n_q), C.byref(dig))
    if name is None:
        raise EngineError("p3hip_create: " + L.p3hip_create_error().decode())
    return name.decode(), n_q.value, dig.value


def debug_graph_table(keys, capacity: int = 64):
    """What a FLAG_LAUNCH_GRAPH_ANY engine's table (csrc/graph_table.h) does with a sequence of passes, feature buffer and
    result target fixed: p3hip_debug_graph_table, no device needed.  keys: (slots, forward rows) pairs, or slot counts
    alone (rows = slots).  Returns (actions, evicted): per pass 0 launched kernel by kernel, 1 captured and launched, 2
    replayed, and the index of the pass whose graph its capture gave up, or -1.  ValueError for a bad argument."""
    L = lib()
    L.p3hip_debug_graph_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    pairs = [(k, k) if np.isscalar(k) else tuple(k) for k in keys]
    npos = np.array([p[0] for p in pairs], np.int32)
    total = np.array([p[1] for p in pairs], np.int32)
    action = np.full(len(pairs), -1, np.int32)
    evicted = np.full(len(pairs), -2, np.int32)
    if L.p3hip_debug_graph_table(npos.ctypes.data, total.ctypes.data, len(pairs), int(capacity), action.ctypes.data,
                                 evicted.ctypes.data) != 0:
        raise ValueError("p3hip_debug_graph_table: bad argument")
    return action.tolist(), evicted.tolist()


def debug_poison_table() -> dict:
    """{device pointer member of p3hip_engine: (class, range that stays zero)} of the table p3hip_debug_poison goes by
    (csrc/engine.cpp kDeviceBuffers; no device needed).  ValueError where a member has two rows."""
    L = lib()
    L.p3hip_debug_poison_table.restype = C.c_char_p
    L.p3hip_debug_poison_table.argtypes = []
    out = {}
    for line in L.p3hip_debug_poison_table().decode().splitlines():
        name, cls, zero_range = line.split("\t")
        if name in out:
            raise ValueError(f"p3hip_debug_poison_table: {name} has two rows")
        out[name] = (cls, zero_range)
    return out


def debug_tfm_split(npos: int, heads: int, n_cu: int = 256):
    """(query parts per (position, head) of the attention launch, tokens per workgroup of qkv and ffn) of a
    FLAG_LOW_LATENCY_TFM engine's launches over npos positions, P3HIP_TFM_SPLIT included: p3hip_debug_tfm_split, no device
    needed.  ValueError for a bad argument or a bad P3HIP_TFM_SPLIT."""
    L = lib()
    L.p3hip_debug_tfm_split.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    s, t = C.c_int(0), C.c_int(0)
    if L.p3hip_debug_tfm_split(npos, heads, n_cu, C.byref(s), C.byref(t)) != 0:
        raise ValueError("p3hip_debug_tfm_split: bad argument or bad P3HIP_TFM_SPLIT")
    return s.value, t.value


def debug_edge_split(npos: int, c_pad: int, n_cu: int = 256):
    """(stem, broadcast dense, heads) parts per position of a low-latency engine's launches around the trunk over npos
    positions of a c_pad-channel stream (csrc/edge_split.h), P3HIP_EDGE_SPLIT included: p3hip_debug_edge_split, no device
    needed.  ValueError for a bad argument or a bad P3HIP_EDGE_SPLIT (the hook then answers 1, 1, 1)."""
    L = lib()
    L.p3hip_debug_edge_split.argtypes = [C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 3
    s, d, h = C.c_int(0), C.c_int(0), C.c_int(0)
    if L.p3hip_debug_edge_split(npos, c_pad, n_cu, C.byref(s), C.byref(d), C.byref(h)) != 0:
        assert (s.value, d.value, h.value) == (1, 1, 1)
        raise ValueError("p3hip_debug_edge_split: bad argument or bad P3HIP_EDGE_SPLIT")
    return s.value, d.value, h.value


def debug_split(npos: int, kw: int, cout: int, n_cu: int = 256):
    """(row strips, output-channel tile) of a k_sconv launch of a FLAG_LOW_LATENCY engine, P3HIP_SPLIT included:
    p3hip_debug_split, no device needed.  ValueError for a bad argument or a bad P3HIP_SPLIT."""
    L = lib()
    L.p3hip_debug_split.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    s, t = C.c_int(0), C.c_int(0)
    if L.p3hip_debug_split(npos, kw, cout, n_cu, C.byref(s), C.byref(t)) != 0:
        raise ValueError("p3hip_debug_split: bad argument or bad P3HIP_SPLIT")
    return s.value, t.value


def pack_sconv(w: np.ndarray, cin_pad: int, cout_pad: int) -> np.ndarray:
    """k_sconv's weight image of w [taps][cin][cout] (csrc/conv_split.h pack_sconv) as float16
    [cout_pad / 16][cin_pad / 32][taps][64][8]; no device needed."""
    w = np.ascontiguousarray(w, np.float32)
    taps, cin, cout = w.shape
    L = lib()
    L.p3hip_debug_pack_sconv.restype = C.c_long
    L.p3hip_debug_pack_sconv.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
    out = np.zeros(taps * cin_pad * cout_pad, np.float16)
    n = L.p3hip_debug_pack_sconv(w.ctypes.data, taps, cin, cout, cin_pad, cout_pad, out.ctypes.data, out.size)
    if n != out.size:
        raise ValueError(f"pack_sconv: the image has {n} elements, expected {out.size}")
    return out.reshape(cout_pad // 16, cin_pad // 32, taps, 64, 8)


def pack_wconv(w: np.ndarray, cin_pad: int, cout_pad: int) -> np.ndarray:
    """k_wconv's weight image of the 3x3 conv w [9][cin][cout] (csrc/conv_wino.h pack_wconv) as float16
    [cout_pad / 16][cin_pad / 32][16 planes][64][8]; no device needed."""
    w = np.ascontiguousarray(w, np.float32)
    taps, cin, cout = w.shape
    if taps != 9:
        raise ValueError("pack_wconv: a 3x3 conv has 9 taps")
    L = lib()
    L.p3hip_debug_pack_wconv.restype = C.c_long
    L.p3hip_debug_pack_wconv.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_long]
    out = np.zeros(16 * cin_pad * cout_pad, np.float16)
    n = L.p3hip_debug_pack_wconv(w.ctypes.data, cin, cout, cin_pad, cout_pad, out.ctypes.data, out.size)
    if n != out.size:
        raise ValueError(f"pack_wconv: the image has {n} elements, expected {out.size}")
    return out.reshape(cout_pad // 16, cin_pad // 32, 16, 64, 8)


def debug_wconv_grid(npos: int, cout: int, n_cu: int = 256, unit: int = -1):
    """How a k_wconv launch of a FLAG_WINOGRAD engine over npos positions and cout output channels is cut on a device of
    n_cu CUs (p3hip_debug_wconv_grid, no device needed): (grid, units), and with 0 <= unit < units
    (grid, units, first flat tile, tiles, first output channel) of that unit.  ValueError for a bad argument."""
    L = lib()
    L.p3hip_debug_wconv_grid.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_long), C.c_long,
                                         C.POINTER(C.c_long), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    grid, units, t0, nt, c0 = C.c_int(0), C.c_long(0), C.c_long(0), C.c_int(0), C.c_int(0)
    if unit < 0:
        if L.p3hip_debug_wconv_grid(npos, cout, n_cu, C.byref(grid), C.byref(units), -1, None, None, None) != 0:
            raise ValueError("p3hip_debug_wconv_grid: bad argument")
        return grid.value, units.value
    if L.p3hip_debug_wconv_grid(npos, cout, n_cu, C.byref(grid), C.byref(units), unit, C.byref(t0), C.byref(nt), C.byref(c0)) != 0:
        raise ValueError("p3hip_debug_wconv_grid: bad argument")
    return grid.value, units.value, t0.value, nt.value, c0.value


def rope_table():
    """The engine's spiral RoPE tables of the transformer trunk, (cos, sin) as [361][32] float64 (no device needed)."""
    cos = np.zeros((361, 32), np.float64)
    sin = np.zeros((361, 32), np.float64)
    L = lib()
    L.p3hip_rope_table.argtypes = [C.c_void_p, C.c_void_p]
    L.p3hip_rope_table.restype = None
    L.p3hip_rope_table(cos.ctypes.data, sin.ctypes.data)
    return cos, sin


def rope_table_dim(head_dim: int):
    """The engine's spiral RoPE tables for head width `head_dim` (32 or 64), (cos, sin) as [361][head_dim] float64 (no
    device needed); ValueError for a width the engine does not run."""
    cos = np.zeros((361, head_dim), np.float64)
    sin = np.zeros((361, head_dim), np.float64)
    L = lib()
    L.p3hip_rope_table_dim.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.p3hip_rope_table_dim.restype = C.c_int
    if L.p3hip_rope_table_dim(int(head_dim), cos.ctypes.data, sin.ctypes.data) != 0:
        raise ValueError(f"the engine has no RoPE table of head width {head_dim} (32 or 64)")
    return cos, sin


def symmetry_maps():
    """The engine's D4 index maps of the 19 x 19 board, (fwd, inv) as [8][361] uint16 (no device needed):
    features move by out[fwd[s][i]] = in[i], outputs come back by out[inv[s][i]] = in[i]."""
    fwd = np.zeros((8, 361), np.uint16)
    inv = np.zeros((8, 361), np.uint16)
    lib().p3hip_symmetry_maps(fwd.ctypes.data, inv.ctypes.data)
    return fwd, inv


def debug_symmetry_rows(masks, rows: int):
    """(first, total) of the table a FLAG_SYMMETRY_SLOT engine uploads for dense slots with these masks (no device
    needed): first[r] = the row at which slot r's copies start, total = the sum of the popcounts.  EngineError where the
    engine refuses the table: no slot, a mask of 0, more than `rows` copies."""
    m = np.ascontiguousarray(masks, np.uint8)
    first = np.zeros(max(len(m), 1), np.int32)
    total = C.c_int(0)
    if lib().p3hip_debug_symmetry_rows(m.ctypes.data, len(m), rows, first.ctypes.data, C.byref(total)) != 0:
        raise EngineError(f"debug_symmetry_rows: refused ({len(m)} slots, {total.value} copies, {rows} rows)")
    return first[:len(m)], total.value


def create_engine(kind: Kind, path: str, batch_size: int, version: int, device: int = 0,
                  flags: int = 0, symmetry_rows: int = 0) -> HipEngine:
    """CreateEngine (engine_factory.cc:56-73); only kHip is served by this package."""
    if kind == Kind.kHip:
        return HipEngine(path, batch_size, version, device, flags, symmetry_rows)
    raise EngineError(f"Unknown Engine Kind {kind!r} (the reference LOG(FATAL)s here)")
