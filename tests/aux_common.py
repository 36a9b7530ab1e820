"""What tests/test_aux_outputs_cpu.py and tests/test_aux_outputs_gpu.py share: the restatement of the fifteen outputs of
P3HIP_FLAG_AUX (include/p3hip.h p3hip_get_aux), its float32 twin, head weights that drive those outputs to trained-net
magnitudes (sharp_aux), the jobs, the error measure and its bounds.

The reference is aux_stages in float64: PolicyHead.call (model.py:783-812) and ValueHead.call (:887-979) restated from
the primitives heads_common.stages uses (oracle.torch_restatement _conv, _dense, _bn, _gpool, _mish) on the same
head_weights, with go, the pooled g and v and the activated p exposed; the CPU test ties the values it shares with
heads_common.stages to that restatement to 1e-12.  The twin is the same function in float32 torch, with the kernels'
softmax form (heads_common.softmax_twin).  The bounds are 15 times what the twin measures against float64 on the CPU
over every job (the recipe of heads_common.BOUNDS); nothing is derived from what an engine returned.

TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import dataclasses
import json
import os
from typing import Dict, Optional

import numpy as np
import torch

import heads_common as hc
from heads_common import F64, te, tr

AUX_LEN = 837
# the record's segments (include/p3hip.h), grouped as the formulas group them
SEGMENTS = (("pi_logits_aux", 0, 362), ("pi_logits_soft", 362, 724), ("q", 724, 727), ("q_err", 727, 729),
            ("q_score", 729, 732), ("q_score_err", 732, 735), ("mcts_dist_logits", 735, 786), ("mcts_dist_probs", 786, 837))
SEG_NAMES = tuple(s[0] for s in SEGMENTS)
GO_COLS = (2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13)   # go's columns in record order from 724 on
PROB_SEGMENT = ("mcts_dist_logits", "mcts_dist_probs")   # the record's one distribution and the logits it is the softmax of

# max |got - want| / max(1, max |want| over the segment) per position: 15 times the float32 twin's worst over every job
# of JOBS, measured on the CPU and rounded up to two digits (test_aux_outputs_cpu.py re-measures the twin and holds every
# constant between 10 and 100 times what it finds).
BOUNDS = {                          # the twin's worst, and the job it was measured on
    "pi_logits_aux": 6.8e-5,        # 4.51e-6 c192v80classic
    "pi_logits_soft": 7.4e-5,       # 4.87e-6 c96v48nbt
    "q": 2.4e-4,                    # 1.56e-5 c384v80nbt
    "q_err": 3.0e-4,                # 1.94e-5 c128v64btl:int8
    "q_score": 2.3e-5,              # 1.50e-6 d96h3v64:fp32
    "q_score_err": 1.1e-4,          # 7.03e-6 c384v80nbt
    "mcts_dist_logits": 2.1e-6,     # 1.34e-7 c96v48nbt
    "mcts_dist_probs": 7.4e-5,      # 4.90e-6 c128v32btl
}
# absolute, on mcts_dist_probs against the float64 softmax of the same float32 logits: the float32 softmax twin's worst
# (heads_common.softmax_twin) over the reference logits of every job, times 15 as above.  The record has this one
# distribution; the aux and soft policies are returned as logits only.
PROB_BOUND = 3.3e-6                 # 2.15e-7 c96v48nbt

# sharp_aux' targets
Q_SPAN = 12.0                      # the tanh inputs go[2..4] span -12 .. +12 over the positions: saturated at both ends
QERR_LO, QERR_HI = -95.0, 25.0     # the third smallest / third largest of go[6], go[7]: the sigmoid's far tail
QSCORE_ERR_SPAN = 6.0              # go[11..13] span -6 .. +6: both signs in front of the abs
MCTS_SHIFT = 100.0                 # every bin logit rides on this: a softmax without max subtraction overflows float32
PEAKED = hc.PEAKED                 # positions whose largest bin / aux move / soft move probability is above 0.9
STEP = hc.STEP


def output_names():
    """the 25 ONNX output names of the network, tests/golden/onnx_output_names.json"""
    with open(os.path.join(hc.ROOT, "tests", "golden", "onnx_output_names.json")) as f:
        return json.load(f)


# ---- jobs ------------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Job:
    net: str          # a key of heads_common.NETS
    family: str       # what the job covers: the head-conv family the measured table groups by
    plan: str = "fp16"   # fp16, fp32 (P3HIP_FLAG_FP32 / P3HIP_FLAG_FP32_TFM by the trunk) or int8 (P3HIP_FLAG_INT8_C128)

    @property
    def name(self):
        return self.net + ("" if self.plan == "fp16" else ":" + self.plan)

    @property
    def fp32(self):
        return self.plan == "fp32"


JOBS = [Job("c128v32btl", "fused heads"), Job("c256v48btl", "fused heads"), Job("c384v80nbt", "k_heads"),
        Job("c192v80classic", "classic"), Job("c96v48nbt", "any-width"), Job("d96h3v64", "transformer"),
        Job("d384h6v80", "transformer"), Job("c256v64nbt", "fp32 conv", "fp32"), Job("d96h3v64", "fp32 transformer", "fp32"),
        Job("c128v64btl", "int8", "int8")]

_WEIGHTS: Dict[str, tuple] = {}


def weights(net, pos=None):
    """(cfg, sharp weights) of a net: heads_common's sharp_heads weights, then sharp_aux, computed once"""
    if net not in _WEIGHTS:
        pos = hc.positions() if pos is None else pos
        cfg, _, W = hc.weights(net, pos)
        _WEIGHTS[net] = (cfg, sharp_aux(cfg, W, pos))
    return _WEIGHTS[net]


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def aux_stages(x, W, dt=F64, mutant=None, convs: Optional[dict] = None):
    """The fifteen aux outputs of the trunk output x (NCHW) as rec [N, 837] in the record's order, with go [N, 14], the
    pooled gp and vp [N, 64] and the activated p [N, 32, 19, 19]; float64 numpy whatever dt computes in.
    W: the weights as the engine holds them (heads_common.head_weights).
    mutant: "moves0" (out_moves channel 0 for channel 1), "soft_pass" (soft_pass without its - 3), "go_shift" (go's
    columns shifted by one), "no_abs" (the score errors without abs), "softmax_nomax" (a float32 softmax without max
    subtraction).  convs: keeps the three head convs of x between calls that change none of their weights."""
    x = torch.as_tensor(x).to(dt)
    N = x.shape[0]
    T = lambda n: tr._t(W[n], dt)
    convs = {} if convs is None else convs
    if not convs:
        convs.update({n: tr._conv(x, T(n)) for n in te.HEAD_CONVS})
    p, v = convs["policy.conv_p.w"], convs["value.conv.w"]
    g = tr._mish(tr._bn(convs["policy.conv_g.w"], W, "policy.gpool_bn", dt))
    gp = tr._gpool(g)
    p = tr._mish(p + tr._dense(gp, W, "policy.gpool_dense", dt)[:, :, None, None])
    pi2 = tr._conv(p, T("policy.out_moves.w")).reshape(N, 2, 361)
    pass2 = tr._dense(gp, W, "policy.out_pass", dt) - 3
    pi_aux = torch.cat([pi2[:, 0 if mutant == "moves0" else 1], pass2[:, 1:2]], dim=1)
    soft = tr._conv(p, T("policy.soft_moves.w")).reshape(N, 361)
    pi_soft = torch.cat([soft, tr._dense(gp, W, "policy.soft_pass", dt) - (0 if mutant == "soft_pass" else 3)], dim=1)
    vp = tr._gpool(v)
    emb = tr._mish(tr._dense(vp, W, "value.oq_embed", dt))
    go = tr._dense(emb, W, "value.oq_out", dt)
    gs = torch.roll(go, 1, dims=1) if mutant == "go_shift" else go
    q = torch.tanh(gs[:, 2:5])
    q_err = 4 * torch.sigmoid(gs[:, 6:8])
    q_score = gs[:, 8:11]
    q_score_err = gs[:, 11:14] if mutant == "no_abs" else torch.abs(gs[:, 11:14])
    ml = tr._dense(emb, W, "value.mcts_dist", dt)
    if mutant == "softmax_nomax":
        mp = torch.from_numpy(hc.softmax_twin(ml.double().numpy(), no_max=True)).to(dt)
    elif dt == torch.float32:
        mp = torch.from_numpy(hc.softmax_twin(ml.numpy())).to(dt)
    else:
        mp = torch.softmax(ml, dim=1)
    rec = torch.cat([pi_aux, pi_soft, q, q_err, q_score, q_score_err, ml, mp], dim=1)
    assert rec.shape[1] == AUX_LEN
    out = dict(rec=rec, go=go, gp=gp, vp=vp, p=p, emb=emb)
    return {k: t.double().numpy() for k, t in out.items()}


def reference(W, x, fp32=False):
    """rec [n, 837] float64 of aux_stages on x, the weights as an engine of that plan holds them"""
    return aux_stages(x, hc.head_weights(W, fp32))["rec"]


def twin_rec(W, x, fp32=False):
    """rec of the float32 twin on x, as float64 numpy"""
    return aux_stages(x, hc.head_weights(W, fp32), dt=torch.float32)["rec"]


# ---- sharp weights -----------------------------------------------------------------------------------------------------------

def sharp_aux(cfg, W, pos):
    """W (heads_common.sharp_heads weights) with the tensors only the aux outputs read at trained-net magnitudes, and
    nothing else changed: columns 0, 1 and 5 of oq_out, channel 0 of out_moves and out_pass keep their values, so every
    output heads_common checks keeps its regime.  Calibrated on the float64 restatement over `pos`, one tensor at a
    time: go[2..4] span +-Q_SPAN (tanh saturated at both ends), go[6..7] reach QERR_LO .. QERR_HI (exp(-s) overflows
    float32 below -88.7), go[11..13] span +-QSCORE_ERR_SPAN, the bin logits ride on MCTS_SHIFT and are raised by factors
    of STEP until PEAKED positions have a bin above 0.9, and so are channel 1 of out_moves and soft_moves for the aux
    and soft move probabilities."""
    W = {k: np.array(v, copy=True) for k, v in W.items()}
    x = hc.trunk_x(cfg, W, pos)
    convs: dict = {}
    st = lambda: aux_stages(x, hc.head_weights(W, False), convs=convs)
    go = st()["go"]
    w, b = np.asarray(W["value.oq_out.w"], np.float64), np.asarray(W["value.oq_out.b"], np.float64)
    for c in GO_COLS:
        if c in (2, 3, 4):
            s, o = hc._affine(go[:, c], -Q_SPAN, Q_SPAN)
        elif c in (6, 7):
            s, o = hc._affine(go[:, c], QERR_LO, QERR_HI, 2)
        elif c in (11, 12, 13):
            s, o = hc._affine(go[:, c], -QSCORE_ERR_SPAN, QSCORE_ERR_SPAN)
        else:
            continue
        w[:, c] *= s
        b[c] = s * b[c] + o
    W["value.oq_out.w"], W["value.oq_out.b"] = w.astype(np.float32), b.astype(np.float32)
    W["value.mcts_dist.b"] = (W["value.mcts_dist.b"].astype(np.float64) + MCTS_SHIFT).astype(np.float32)

    def raise_until(names, peaked):
        nonlocal W
        W0, scale = W, 1.0
        for _ in range(80):
            W = dict(W0)
            for n, ch in names:
                t = W0[n].astype(np.float64)
                if ch is None:
                    t = t * scale
                else:
                    t[..., ch] *= scale
                W[n] = t.astype(np.float32)
            if peaked(st()["rec"]) >= PEAKED:
                return
            scale *= STEP
        raise AssertionError(f"sharp_aux: {names} did not reach {PEAKED} peaked positions")

    top = lambda a, b_: lambda rec: int((hc.softmax64(rec[:, a:b_]).max(axis=1) > 0.9).sum())
    raise_until([("value.mcts_dist.w", None)], top(735, 786))
    raise_until([("policy.out_moves.w", 1)], top(0, 362))
    raise_until([("policy.soft_moves.w", None)], top(362, 724))
    return W


def coverage(rec64, st):
    """positions per regime of a float64 reference (rec64 [n, 837], st = aux_stages(...))"""
    go = st["go"]
    return {
        "tanh saturated high": int((go[:, 2:5].max(axis=1) > 9).sum()), "tanh saturated low": int((go[:, 2:5].min(axis=1) < -9).sum()),
        "q_err logit < -89": int((go[:, 6:8].min(axis=1) < -89).sum()), "q_err logit > 20": int((go[:, 6:8].max(axis=1) > 20).sum()),
        "score err negative": int((go[:, 11:14].min(axis=1) < -1).sum()), "score err positive": int((go[:, 11:14].max(axis=1) > 1).sum()),
        "bin logit > 89": int((rec64[:, 735:786].max(axis=1) > 89).sum()),
        "bin > 0.9": int((rec64[:, 786:837].max(axis=1) > 0.9).sum()),
        "aux move > 0.9": int((hc.softmax64(rec64[:, 0:362]).max(axis=1) > 0.9).sum()),
        "soft move > 0.9": int((hc.softmax64(rec64[:, 362:724]).max(axis=1) > 0.9).sum()),
        "finite": bool(np.isfinite(rec64).all()),
    }


COVERAGE_MIN = {"tanh saturated high": 1, "tanh saturated low": 1, "q_err logit < -89": 1, "q_err logit > 20": 1,
                "score err negative": 2, "score err positive": 2, "bin logit > 89": hc.BATCH, "bin > 0.9": 2,
                "aux move > 0.9": 2, "soft move > 0.9": 2}


def assert_coverage(c, label):
    assert c["finite"], label
    for k, n in COVERAGE_MIN.items():
        assert c[k] >= n, (label, k, c[k], c)


# ---- the measure and the checks ------------------------------------------------------------------------------------------------

def segment_errors(got, want):
    """{segment: [n] max |got - want| / max(1, max |want|) per position}; a non-finite got counts as inf"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and got.shape[1] == AUX_LEN, (got.shape, want.shape)
    out = {}
    for name, a, b in SEGMENTS:
        d = np.abs(got[:, a:b] - want[:, a:b])
        d = np.where(np.isfinite(got[:, a:b]), d, np.inf)
        out[name] = d.max(axis=1) / np.maximum(1.0, np.abs(want[:, a:b]).max(axis=1))
    return out


def worst(errs):
    return {k: float(v.max()) for k, v in errs.items()}


def prob_errors(rec):
    """[n] max |mcts_dist_probs - float64 softmax of the record's own float32 mcts_dist_logits|; non-finite: inf"""
    rec = np.asarray(rec)
    logits = rec[:, 735:786].astype(np.float32).astype(np.float64)
    got = rec[:, 786:837].astype(np.float64)
    d = np.where(np.isfinite(got), np.abs(got - hc.softmax64(logits)), np.inf)
    return d.max(axis=1)


def check_rec(job, got, want, bounds=None, prob_bound=None):
    """every segment of every position inside its bound, and the distribution inside PROB_BOUND of the softmax of its own
    logits; returns the worst per segment (and "softmax").  No position is left out: got and want have one row each."""
    bounds = BOUNDS if bounds is None else bounds
    prob_bound = PROB_BOUND if prob_bound is None else prob_bound
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    errs = segment_errors(got, want)
    for name, a, b in SEGMENTS:
        n = int(errs[name].argmax())
        if not errs[name][n] <= bounds[name]:
            d = np.where(np.isfinite(got[n, a:b]), np.abs(got[n, a:b] - want[n, a:b]), np.inf)
            i = int(d.argmax())
            over = [int(s) for s in np.nonzero(~(errs[name] <= bounds[name]))[0]]
            raise AssertionError(
                f"{job}: segment {name} error {errs[name][n]:.3g} over its bound {bounds[name]:.3g} at slot {n} index {i}: "
                f"got {got[n, a + i]!r} want {want[n, a + i]!r} (segment max |want| {np.abs(want[n, a:b]).max():.4g}); "
                f"slots over the bound {over[:16]}")
    pe = prob_errors(got)
    n = int(pe.argmax())
    if not pe[n] <= prob_bound:
        raise AssertionError(f"{job}: mcts_dist_probs of slot {n} is {pe[n]:.3g} from the softmax of its own logits, over "
                             f"{prob_bound:.3g} (largest logit {got[n, 735:786].max()!r}, sum {got[n, 786:837].sum()!r})")
    out = worst(errs)
    out["softmax"] = float(pe.max())
    return out
