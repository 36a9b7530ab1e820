"""What tests/test_heads_cpu.py and tests/test_heads_gpu.py share: head weights at trained-net magnitudes (sharp_heads),
the one-block nets and jobs that reach every instantiation of the head kernels (kernels.hip k_headsx<C,32,V>,
k_heads<32,V>, the fp32 plans' k_heads), the restatement of the heads stage by stage with its mutants, the regime
counter, the error measure with its bounds, and the check of the result record.

The reference is the float64 restatement of the heads (tfm_restatement._heads, through trunk_emulation.Trunk.heads) on
the x the heads got; stages() below is the same arithmetic with its intermediate values exposed (the CPU test ties the
two together to 1e-12).  The bounds are ten times what a float32 twin of the heads measures against float64 on the CPU
over every job; nothing is derived from what an engine returned.

The twin (twin_raw) is trunk_emulation.Trunk(twin=True).heads: the same restatement in float32 torch arithmetic (on the
fp32 jobs without the fp16 rounding of the head convs).  Its error is float32 rounding and summation order at these
magnitudes: mish outputs of up to 30 times weights of order one sum to gamma and to the score logits with cancellation.

TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import dataclasses
import os
import sys
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import torch_restatement as tr  # noqa: E402
import tfm_restatement_dh as dh  # noqa: E402
import trunk_emulation as te  # noqa: E402

F64 = torch.float64
BATCH = 41   # a ragged tail for k_heads' four-position and k_headsx' two-position workgroups
SEGMENTS = (("pi", 0, 362), ("opt", 362, 724), ("outcome", 724, 726), ("score", 726, 1526), ("ownership", 1526, 1887),
            ("q6_err", 1887, 1888), ("gamma", 1888, 1889))   # p3hip_get_raw
SEG_NAMES = tuple(s[0] for s in SEGMENTS)
MISH_INPUTS = ("policy.gpool_dense", "value.oq_embed", "value.gamma_pre", "value.score_pre")
PROB_KEYS = ("move_probs", "opt_move_probs", "score_probs", "value_probs")
PROB_SLICES = {"move_probs": (0, 362), "opt_move_probs": (362, 724), "score_probs": (726, 1526), "value_probs": (724, 726)}

# max |got - want| / max(1, max |want| over the segment) per position.  The rule is ten times the twin's worst over
# every job of JOBS; the constants are 15 times the figure measured (AVX-512 torch kernels), rounded up to two digits,
# because that figure is a maximum of float32 rounding noise and moves with the CPU's vector width: with AVX2 kernels
# score measured 7.74e-5 (+14 %), opt 8.61e-6, pi 5.35e-6.  test_heads_cpu.py re-measures the twin and holds every
# constant between 10 and 100 times what it finds.
BOUNDS = {                  # the twin's worst, and the job it was measured on
    "pi": 8.8e-5,           # 5.84e-6 c256v64nbt:fp32
    "opt": 1.3e-4,          # 8.47e-6 c128v64btl
    "outcome": 4.4e-5,      # 2.87e-6 c512v80nbt
    "score": 1.1e-3,        # 6.81e-5 c256v48btl
    "ownership": 3.6e-4,    # 2.38e-5 c384v80nbt:fp32
    "q6_err": 1.6e-3,       # 1.04e-4 c128v64btl
    "gamma": 9.5e-4,        # 6.31e-5 c384v32btl
}
# absolute, on the probabilities of the record against the float64 softmax of the same float32 logits: the float32
# softmax twin's worst (softmax_twin) over the reference logits of every job, times 15 as above
PROB_BOUNDS = {
    "move_probs": 3.9e-6,       # 2.57e-7 d192h6v64
    "opt_move_probs": 4.9e-6,   # 3.22e-7 c256v48btl
    "score_probs": 2.6e-6,      # 1.69e-7 c192v80classic
    "value_probs": 1.4e-6,      # 8.68e-8 c384v80nbt:hot
}

# sharp_heads' targets
MISH_SPAN = 30.0          # the output of every head layer in front of a mish spans -30 .. +30 over the positions
GAMMA_LO, GAMMA_HI = -8.0, 25.0     # the third smallest / third largest gamma
Q6_LO, Q6_HI = -95.0, 25.0          # the third smallest / third largest q6_err logit
OUTCOME_DIFF = 40.0       # the fourth smallest / largest outcome-logit difference: -40 / +40
OUTCOME_SHIFT = 100.0     # both outcome logits ride on this: a softmax without max subtraction overflows float32
OWN_PEAK, OWN_TYPICAL = 12.0, 3.0   # median over positions of the largest |pre-tanh|; median |pre-tanh| over all points
PEAKED = 8                # positions whose largest move / opt / score probability is above 0.9
STEP = 1.25               # peak_policy's and score_out's scale grow by this factor until PEAKED positions are


# ---- nets and jobs -------------------------------------------------------------------------------------------------

def _nets():
    from p3achygo_amd.netspec import NetConfig, transformer_config
    c = lambda name, C, Cb, V, inner, kind: NetConfig(name, 1, C, Cb, 32, V, 3, inner, kind)
    nets = [c("c128v32btl", 128, 64, 32, 2, "btl"), c("c128v48nbt", 128, 64, 48, 2, "nbt"),
            c("c128v64btl", 128, 64, 64, 1, "btl"), c("c256v32nbt", 256, 128, 32, 2, "nbt"),
            c("c256v48btl", 256, 128, 48, 3, "btl"), c("c256v64nbt", 256, 128, 64, 2, "nbt"),
            c("c384v32btl", 384, 192, 32, 2, "btl"), c("c384v48nbt", 384, 192, 48, 2, "nbt"),
            c("c384v64btl", 384, 192, 64, 3, "btl"), c("c384v80nbt", 384, 192, 80, 2, "nbt"),
            c("c192v80classic", 192, 64, 80, 2, "classic"),
            c("c64v32btl", 64, 32, 32, 2, "btl"), c("c512v80nbt", 512, 256, 80, 2, "nbt"),
            c("c96v48nbt", 96, 48, 48, 2, "nbt"),                      # C and C_b padded (128, 64)
            transformer_config("d96h3v64", 1, 96, 3), transformer_config("d192h6v64", 1, 192, 6),
            transformer_config("d384h6v80", 1, 384, 6, c_val=80)]
    return {n.name: n for n in nets}


NETS = _nets()
FUSABLE = ["c128v32btl", "c128v48nbt", "c128v64btl", "c256v32nbt", "c256v48btl", "c256v64nbt"]
HOT = ["c256v64nbt:hot", "c384v80nbt:hot"]      # trunk_emulation.hot_weights, then sharp_heads


@dataclasses.dataclass(frozen=True)
class Job:
    net: str          # a key of NETS, with ":hot" for hot_weights under the sharp heads
    family: str       # k_headsx, k_heads or fp32: the kernel family the measured table groups by
    fp32: bool = False
    env: str = ""     # "" or "P3HIP_NO_HFUSE": the child process the job runs in

    @property
    def name(self):
        return self.net + (":fp32" if self.fp32 else "") + (":nohfuse" if self.env else "")


JOBS = ([Job(n, "k_headsx") for n in FUSABLE] +
        [Job(n, "k_heads") for n in ("c384v32btl", "c384v48nbt", "c384v64btl", "c384v80nbt", "c192v80classic")] +
        [Job(n, "k_heads", env="P3HIP_NO_HFUSE") for n in FUSABLE] +
        [Job(n, "k_heads") for n in ("c64v32btl", "c512v80nbt", "c96v48nbt")] +          # the any-width kernels
        [Job("c256v64nbt", "fp32", fp32=True), Job("c384v80nbt", "fp32", fp32=True), Job("d96h3v64", "fp32", fp32=True)] +
        [Job("d96h3v64", "k_headsx"), Job("d192h6v64", "k_headsx"), Job("d384h6v80", "k_heads")] +
        [Job(HOT[0], "k_headsx"), Job(HOT[1], "k_heads")])


def config(net):
    return NETS[net.partition(":")[0]]


def is_tfm(cfg):
    return cfg.block_type == "transformer"


def stream_width(cfg):
    """the channels p3hip_debug_x returns for cfg: transformers padded to 128 / 256 / 384, conv trunks to 64s"""
    C = cfg.channels
    if is_tfm(cfg):
        return 128 if C <= 128 else (256 if C <= 256 else 384)
    return (C + 63) // 64 * 64


def positions():
    """BATCH positions: test_trunk_blocks_gpu.handmade_positions scattered among seeded fill"""
    from p3achygo_amd import features
    from test_trunk_blocks_gpu import handmade_positions
    pos = features.random_positions(BATCH, seed=43, n_games=16, max_moves=300, komis=(7.5, -7.5, 0.5))
    special = handmade_positions()
    pos[[int(s) for s in np.linspace(0, BATCH - 1, len(special)).round()]] = special
    return pos


def trunk_x(cfg, W, pos, fp16=True):
    """the trunk output of the restatement (fp16: rounded where the engine stores fp16) as float64 NCHW"""
    if is_tfm(cfg):
        planes, sc = te.inputs(pos)
        t = dh.forward(cfg, W, planes, sc, fp16=fp16)["trunk"]
        return torch.from_numpy(np.ascontiguousarray(t.reshape(len(pos), 19, 19, cfg.channels).transpose(0, 3, 1, 2)))
    return te.Trunk(cfg, W, fp16=fp16).trunk(pos)[-1]


_WEIGHTS: Dict[str, tuple] = {}


def weights(net, pos=None):
    """(cfg, ordinary weights, sharp weights) of a net name, computed once; sharp: calibrated on positions()"""
    if net not in _WEIGHTS:
        from p3achygo_amd import netspec
        cfg = config(net)
        pos = positions() if pos is None else pos
        W0 = netspec.generate_weights(cfg, randomize=True)
        if is_tfm(cfg):
            for i in range(cfg.blocks):
                for n in ("q", "k"):
                    W0[f"blocks.{i}.{n}.w"] = (W0[f"blocks.{i}.{n}.w"] * np.float32(1.5)).astype(np.float32)
        if net.endswith(":hot"):
            W0 = te.hot_weights(cfg, W0, pos)
        _WEIGHTS[net] = (cfg, W0, sharp_heads(cfg, W0, pos))
    return _WEIGHTS[net]


def head_weights(W, fp32):
    """the head weights as the engine holds them: the three head convs fp16-rounded on an fp16 engine"""
    if fp32:
        return W
    return {k: (v.astype(np.float16).astype(np.float32) if k in te.HEAD_CONVS else v) for k, v in W.items()}


def reference(cfg, W, x, fp32=False):
    """raw [n, 1889] float64 of heads() on x: trunk_emulation.Trunk.heads (tfm_restatement._heads)"""
    return te.Trunk(cfg, W, fp16=not fp32).heads(torch.as_tensor(x, dtype=F64))


# ---- the heads stage by stage ------------------------------------------------------------------------------------------

def stages(x, W, dt=F64, mutant=None, convs: Optional[dict] = None):
    """PolicyHead.call and ValueHead.call as tfm_restatement._heads states them, with the intermediate values kept.
    x: NCHW; W: the weights as the engine holds them (head_weights).  mutant: 1 - 6, 3b and 8 of tests/test_heads_cpu.py.
    Returns a dict of float64 numpy arrays: raw and gamma, softplus, factor (the clamped softplus), own_pre, go, and per
    head mish layer mish:<layer> (the mish input) and dense:<layer> (the layer's own output in it).
    convs: a dict that keeps the three head convs of x between calls that change none of their weights."""
    x = torch.as_tensor(x).to(dt)
    N = x.shape[0]
    T = lambda n: tr._t(W[n], dt)
    mish = tr._mish
    out = {}
    convs = {} if convs is None else convs
    if not convs:
        convs.update({n: tr._conv(x, T(n)) for n in te.HEAD_CONVS})
    p, v = convs["policy.conv_p.w"], convs["value.conv.w"]
    g = mish(tr._bn(convs["policy.conv_g.w"], W, "policy.gpool_bn", dt))
    gp = tr._gpool(g)
    z = p + tr._dense(gp, W, "policy.gpool_dense", dt)[:, :, None, None]
    out["mish:policy.gpool_dense"], out["dense:policy.gpool_dense"] = z, z[:, :, 0, 0] - p[:, :, 0, 0]
    p = mish(z)
    pi2 = tr._conv(p, T("policy.out_moves.w")).reshape(N, 2, 361)
    pass2 = tr._dense(gp, W, "policy.out_pass", dt) - (0 if mutant == 8 else 3)
    pi_logits = torch.cat([pi2[:, 0], pass2[:, 0:1]], dim=1)
    opt = tr._conv(p, T("policy.opt_moves.w")).reshape(N, 361)
    opt_logits = torch.cat([opt, tr._dense(gp, W, "policy.opt_pass", dt) - 3], dim=1)
    vp = tr._gpool(v)
    z = tr._dense(vp, W, "value.oq_embed", dt)
    out["mish:value.oq_embed"] = out["dense:value.oq_embed"] = z
    go = tr._dense(mish(z), W, "value.oq_out", dt)
    own_pre = tr._conv(v, T("value.own.w")).reshape(N, 361)
    own = torch.clamp(own_pre, -1.0, 1.0) if mutant == 5 else torch.tanh(own_pre)
    z = tr._dense(vp, W, "value.gamma_pre", dt)
    out["mish:value.gamma_pre"] = out["dense:value.gamma_pre"] = z
    gamma = tr._dense(mish(z), W, "value.gamma_out", dt)
    scores = 0.05 * torch.arange(-399 if mutant == 4 else -400, 401 if mutant == 4 else 400, dtype=dt) + 0.025
    vs = torch.cat([vp[:, None, :].expand(N, 800, vp.shape[1]), scores[None, :, None].expand(N, 800, 1)], dim=2)
    z = tr._dense(vs, W, "value.score_pre", dt)
    out["mish:value.score_pre"] = out["dense:value.score_pre"] = z
    sl = tr._dense(mish(z), W, "value.score_out", dt).reshape(N, 800)
    if mutant == 2:
        sp = torch.clamp(gamma, min=0.0)
    elif mutant == 3:   # the > 20 branch returns log1p(exp(20))
        sp = torch.where(gamma > 20.0, torch.full_like(gamma, float(np.log1p(np.exp(20.0)))),
                         F.softplus(torch.clamp(gamma, max=20.0)))
    elif mutant == "3b":   # the > 20 branch returns log1p(exp(-s)): the stable form s + log1p(exp(-s)) without its s
        sp = torch.where(gamma > 20.0, torch.log1p(torch.exp(-torch.clamp(gamma, min=20.0))),
                         F.softplus(torch.clamp(gamma, max=20.0)))
    else:
        sp = F.softplus(gamma)
    factor = sp if mutant == 1 else torch.clamp(sp, max=10.0)
    score_logits = factor * sl
    s5 = go[:, 5:6]
    if mutant == 6:     # float32, sigmoid(s) = 1 - e / (1 + e), e = exp(-s): inf / inf below -88.7
        e = torch.exp(-s5.float())
        q6 = (4.0 * (1.0 - e / (1.0 + e))).to(dt)
    else:
        q6 = 4 * torch.sigmoid(s5)
    raw = torch.cat([pi_logits, opt_logits, go[:, 0:2], score_logits, own, q6, gamma], dim=1)
    out.update(raw=raw, gamma=gamma[:, 0], softplus=sp[:, 0], factor=factor[:, 0], own_pre=own_pre, go=go)
    return {k: v_.double().numpy() for k, v_ in out.items()}


def twin_raw(cfg, W, x, fp32=False):
    """raw of the float32 twin (module docstring) on x, as float64 numpy"""
    t = te.Trunk(cfg, W, twin=True)
    t.fp16 = not fp32
    return np.asarray(t.heads(torch.as_tensor(x, dtype=F64)), np.float64)


def softmax64(logits):
    l = np.asarray(logits, np.float64)
    e = np.exp(l - l.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def softmax_twin(logits, no_max=False):
    """the kernels' softmax in float32 torch: 2^((l - max) log2 e) / sum.  no_max: mutant 7, exp(l) / sum"""
    l = torch.from_numpy(np.asarray(logits, np.float32))
    e = torch.exp(l) if no_max else torch.exp2((l - l.amax(-1, keepdim=True)) * np.float32(te.LOG2E))
    return (e / e.sum(-1, keepdim=True)).double().numpy()


def probs64(raw):
    """the four distributions of the record from raw logits ([n, 1889] or [1889]), float64"""
    raw = np.asarray(raw)
    return {k: softmax64(raw[..., a:b]) for k, (a, b) in PROB_SLICES.items()}


# ---- sharp head weights ----------------------------------------------------------------------------------------------------

def _affine(d, lo, hi, k=0):
    """(s, b): s d + b puts the k-th smallest value of d at lo and the k-th largest at hi"""
    v = np.sort(np.asarray(d, np.float64).ravel())
    s = (hi - lo) / (v[-1 - k] - v[k])
    return s, lo - s * v[k]


def _scaled(W, name, s, b=None):
    """the layer's output y becomes s y + b"""
    W[name + ".w"] = (np.asarray(W[name + ".w"], np.float64) * s).astype(np.float32)
    if b is not None:
        W[name + ".b"] = (np.asarray(W[name + ".b"], np.float64) * s + b).astype(np.float32)


def sharp_heads(cfg, W, pos):
    """W with the head tensors at trained-net magnitudes and nothing else changed.  One tensor at a time, in the order
    the heads apply them, each calibrated on the float64 restatement over `pos` (as trunk_emulation.hot_weights does
    for the trunk): the four head mish inputs span +-MISH_SPAN; gamma spans GAMMA_LO .. GAMMA_HI (both signs, past the
    clamp at 10 and the branch at 20); the q6_err logit spans Q6_LO .. Q6_HI; the outcome difference +-OUTCOME_DIFF on
    logits near OUTCOME_SHIFT; ownership saturates; netspec.peak_policy and score_out are raised by factors of STEP until
    PEAKED positions have a largest probability above 0.9."""
    from p3achygo_amd import netspec
    W = {k: np.array(v, copy=True) for k, v in W.items()}
    x = trunk_x(cfg, W, pos)
    convs: dict = {}
    st = lambda: stages(x, head_weights(W, False), convs=convs)

    def mish_layer(name):   # the layer's own output spans +-MISH_SPAN (the policy's mish adds conv_p's to it)
        _scaled(W, name, *_affine(st()["dense:" + name], -MISH_SPAN, MISH_SPAN))

    mish_layer("policy.gpool_dense")
    # peaked policy and optimistic policy
    W0, scale = W, 1.0
    for _ in range(60):
        W = netspec.peak_policy(W0, scale)
        pr = probs64(st()["raw"])
        if min((pr[k].max(axis=1) > 0.9).sum() for k in ("move_probs", "opt_move_probs")) >= PEAKED:
            break
        scale *= STEP
    W = {k: np.array(v, copy=True) for k, v in W.items()}
    mish_layer("value.oq_embed")
    go = st()["go"]
    d = go[:, 0] - go[:, 1]
    sd, _ = _affine(d, -OUTCOME_DIFF, OUTCOME_DIFF, 3)
    s5, b5 = _affine(go[:, 5], Q6_LO, Q6_HI, 2)
    w = np.asarray(W["value.oq_out.w"], np.float64)
    w[:, 0:2] *= sd
    w[:, 5] *= s5
    W["value.oq_out.w"] = w.astype(np.float32)
    W["value.oq_out.b"][5] = np.float32(s5 * W["value.oq_out.b"][5] + b5)
    W["value.oq_out.b"][0:2] = 0
    go = st()["go"]
    d = np.sort(go[:, 0] - go[:, 1])
    W["value.oq_out.b"][0] = np.float32(OUTCOME_SHIFT - (d[3] + d[-4]) / 2 - np.median(go[:, 1]))
    W["value.oq_out.b"][1] = np.float32(OUTCOME_SHIFT - np.median(go[:, 1]))
    a = np.abs(st()["own_pre"])
    _scaled(W, "value.own", max(OWN_PEAK / np.median(a.max(axis=1)), OWN_TYPICAL / np.median(a)))
    mish_layer("value.gamma_pre")
    _scaled(W, "value.gamma_out", *_affine(st()["gamma"], GAMMA_LO, GAMMA_HI, 2))
    mish_layer("value.score_pre")
    # score_out: where both ends of the score curve fall (the largest logit in the interior for every position) the
    # sign is turned, so that the top bin lies at an end of the grid for most positions
    top = probs64(st()["raw"])["score_probs"].argmax(axis=1)
    W0, scale = W, 1.0 if ((top < 32) | (top >= 768)).sum() >= 4 else -1.0
    for _ in range(60):
        W = dict(W0)
        for f in (".w", ".b"):
            W["value.score_out" + f] = (W0["value.score_out" + f].astype(np.float64) * scale).astype(np.float32)
        if (probs64(st()["raw"])["score_probs"].max(axis=1) > 0.9).sum() >= PEAKED:
            break
        scale *= STEP
    return W


# ---- regimes -------------------------------------------------------------------------------------------------------------

def coverage(raw64, probs, st=None):
    """positions per regime of a float64 reference: raw64 [n, 1889], probs = probs64(raw64); st = stages(...) adds the
    pre-activation regimes (the q6_err logit, ownership before tanh, the mish inputs)"""
    raw64 = np.asarray(raw64, np.float64)
    gamma = raw64[:, 1888]
    sp = np.logaddexp(0.0, gamma)
    d = raw64[:, 724] - raw64[:, 725]
    top = probs["score_probs"].argmax(axis=1)
    c = {
        "gamma<-5": int((gamma < -5).sum()),
        "gamma>0,sp<10": int(((gamma > 0) & (sp < 10)).sum()),
        "sp>=10,gamma<=20": int(((sp >= 10) & (gamma <= 20)).sum()),
        "gamma>20": int((gamma > 20).sum()),
        "diff>30": int((d > 30).sum()), "diff<-30": int((d < -30).sum()),
        "pi>0.9": int((probs["move_probs"].max(axis=1) > 0.9).sum()),
        "opt>0.9": int((probs["opt_move_probs"].max(axis=1) > 0.9).sum()),
        "score>0.9": int((probs["score_probs"].max(axis=1) > 0.9).sum()),
        "score top bin in the outer 32": int(((top < 32) | (top >= 768)).sum()),
        "finite": bool(np.isfinite(raw64).all()),
    }
    if st is not None:
        c["q6<-89"] = int((st["go"][:, 5] < -89).sum())
        c["q6>20"] = int((st["go"][:, 5] > 20).sum())
        c["own>9"] = int((np.abs(st["own_pre"]).max(axis=1) > 9).sum())
        for n in MISH_INPUTS:
            z = st["mish:" + n]
            c[f"{n}<-20"], c[f"{n}>20"] = bool(z.min() < -20), bool(z.max() > 20)
    return c


COVERAGE_MIN = {"gamma<-5": 2, "gamma>0,sp<10": 2, "sp>=10,gamma<=20": 2, "gamma>20": 2, "diff>30": 1, "diff<-30": 1,
                "pi>0.9": 2, "opt>0.9": 2, "score>0.9": 2, "score top bin in the outer 32": 2, "q6<-89": 1, "q6>20": 1,
                "own>9": 2}


def assert_coverage(c, label):
    """the conditions of the issue on a coverage() count"""
    assert c["finite"], label
    for k, n in COVERAGE_MIN.items():
        if k in c:
            assert c[k] >= n, (label, k, c[k], c)
    assert c["diff>30"] + c["diff<-30"] >= 2, (label, c)
    for n in MISH_INPUTS:
        for k in (f"{n}<-20", f"{n}>20"):
            assert c.get(k, True), (label, k)


# ---- the measure and the checks ----------------------------------------------------------------------------------------

def segment_errors(got, want):
    """{segment: [n] max |got - want| / max(1, max |want|) per position}; a non-finite got counts as inf"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    out = {}
    for name, a, b in SEGMENTS:
        d = np.abs(got[:, a:b] - want[:, a:b])
        d = np.where(np.isfinite(got[:, a:b]), d, np.inf)
        out[name] = d.max(axis=1) / np.maximum(1.0, np.abs(want[:, a:b]).max(axis=1))
    return out


def worst(errs):
    return {k: float(v.max()) for k, v in errs.items()}


def regime(want_row):
    g = float(want_row[1888])
    sp = float(np.logaddexp(0.0, g))
    return f"gamma {g:.4g} softplus {sp:.4g} {'clamped to 10' if sp > 10 else 'not clamped'}{', past the branch at 20' if g > 20 else ''}"


def check_raw(job, got, want, slots=None, bounds=None):
    """every segment of every position inside its bound; returns the worst per segment.  The message names the job, the
    segment, the slot, the index within the segment, got, want and the position's regime."""
    bounds = BOUNDS if bounds is None else bounds
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    errs = segment_errors(got, want)
    for name, a, b in SEGMENTS:
        n = int(errs[name].argmax())
        if not errs[name][n] <= bounds[name]:
            d = np.where(np.isfinite(got[n, a:b]), np.abs(got[n, a:b] - want[n, a:b]), np.inf)
            i = int(d.argmax())
            over = [int(s if slots is None else slots[s]) for s in np.nonzero(~(errs[name] <= bounds[name]))[0]]
            raise AssertionError(
                f"{job}: segment {name} error {errs[name][n]:.3g} over its bound {bounds[name]:.3g} at slot "
                f"{n if slots is None else slots[n]} index {i}: got {got[n, a + i]!r} want {want[n, a + i]!r} "
                f"(segment max |want| {np.abs(want[n, a:b]).max():.4g}); {regime(want[n])}; slots over the bound {over[:16]}")
    return worst(errs)


def record_check(raw_engine, record, label="", bounds=None):
    """One slot's result record (features.result_to_dict) against the engine's own raw logits of that slot.  Returns the
    largest probability error per distribution."""
    bounds = PROB_BOUNDS if bounds is None else bounds
    raw32 = np.asarray(raw_engine, np.float32)
    want = probs64(raw32.astype(np.float64))
    out = {}
    for k in PROB_KEYS:
        got = np.asarray(record[k], np.float64)
        assert np.isfinite(got).all(), f"{label}: {k} is not finite: {got[~np.isfinite(got)][:4]}"
        d = np.abs(got - want[k])
        i = int(d.argmax())
        assert d[i] <= bounds[k], (f"{label}: {k}[{i}] got {got[i]!r} want {want[k][i]!r}, error {d[i]:.3g} over "
                                   f"{bounds[k]:.3g}; largest logit {raw32[slice(*PROB_SLICES[k])].max()!r}")
        assert abs(got.sum() - 1.0) <= bounds[k] * len(got), f"{label}: {k} sums to {got.sum()!r}"
        out[k] = float(d[i])
    assert np.float32(record["err2_outcome"]).tobytes() == raw32[1887].tobytes(), (label, record["err2_outcome"], raw32[1887])
    assert np.array_equal(np.asarray(record["move_logits"], np.float32).view(np.uint32), raw32[:362].view(np.uint32)), label
    return out
