"""The transformer trunks kernel by kernel against the fp16 emulation (tests/tfm_emulation.py), with teacher forcing:
for block n the engine's own x_n (engine stopped in front of block n, P3HIP_DEBUG_STOP_BLOCK, p3hip_debug_x) and its own
q, k, v, o and x_(n+1) (engine stopped in front of block n + 1, p3hip_debug_tfm; the stop value equal to the block count
ends the pass in front of the heads, which would take o's buffer as scratch) are compared as
    k_tfm_qkv:  qkv(x_n)      against q, k, v
    k_tfm_attn: attn(q, k, v) against o
    k_tfm_ffn:  ffn(o, x_n)   against x_(n+1)
and the stem against x_0, by tfm_emulation.check_kernel with the bounds the twin set on the CPU
(tests/test_transformer_emulation_cpu.py).  Also held, over every position of the batch and not only the compared
slots: rows 361..383 of q, k, v are exactly zero after the first run, after a second run of the same engine with fewer
slots loaded (compaction) and after a third with all of them; channels d..Cs-1 of x are exactly zero after every
block; nothing is NaN or inf.

Each group of jobs runs in one child process under its own time limit; a failing child fails the test, nothing retries,
and nothing else is started after it in that test.  Measured wall time of the children on one MI355X: see CHILD_LIMITS.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tfm_emulation as T  # noqa: E402
import tfm_restatement_dh as dh  # noqa: E402
from conftest import ROOT, load_golden  # noqa: E402
from test_trunk_blocks_gpu import _batch, handmade_positions  # noqa: E402,F401

pytestmark = pytest.mark.gpu

# (net, batch): the eight transformer fixtures (d = 64 .. 384, head width 32 and 64, stream widths 128, 256, 384;
# b14d96h3_transformer with all 14 blocks) at batches of 1 (361 tokens: five full 64-token tiles and a ragged one of
# 41), 7 and 61 (token tiles span two positions) and 300 (more attention workgroups than CUs)
PLAIN_JOBS = [("test_b2d96h3_tfm", 1), ("b14d96h3_transformer", 7), ("test_b2d64h2_tfm", 61), ("test_b2d128h2_tfm", 300),
              ("test_b2d192h6_tfm", 7), ("test_b2d256h4_tfm", 61), ("test_b2d384h12_tfm", 300), ("test_b2d384h6_tfm", 1)]
# hot (tfm_emulation.hot_weights: Wq, Wk x 4): one net per (attention path, FFN path, stream width) the fixtures have:
# D = 32 with x1 in LDS (d = 96, Cs = 128); D = 64 and D = 32 with x1 in registers at Cs = 128 / 256 / 384 (no
# supported width has D = 64 and d <= 96 but d = 64 with one head, which has no fixture).  :m1: the engine gets weights
# the emulation does not.
HOT_JOBS = [("test_b2d96h3_tfm:hot", 61), ("test_b2d128h2_tfm:hot", 7), ("test_b2d192h6_tfm:hot", 61),
            ("test_b2d256h4_tfm:hot", 300), ("test_b2d384h12_tfm:hot", 7), ("test_b2d384h6_tfm:hot", 61),
            ("test_b2d96h3_tfm:m1", 7)]
M1 = dict(block=1, head=1, lanes=(6, 7))   # Wk of block 1: two adjacent output channels of head 1 exchanged
# time limit of each child, s; measured on one MI355X: plain 6 s (36 engines), hot 4 s (25 engines).  The limit leaves
# room for a cold start of the runtime and a loaded machine.
CHILD_LIMITS = {"plain": 300, "hot": 300}

_CHILD = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np
from p3achygo_amd import engine, features
d = np.load(sys.argv[1], allow_pickle=True)
out = {}
def zero_rows(eng, n, heads, D):
    ok = True
    for w in range(3):
        a = eng.debug_tfm(w, n, heads, D)
        ok = ok and bool((a[:, :, 361:] == 0).all()) and bool(np.isfinite(a).all())
    return ok
for key in d["keys"]:
    path, Cs, dm, heads, nblk = d[key + ":path"].item(), int(d[key + ":Cs"]), int(d[key + ":d"]), int(d[key + ":heads"]), int(d[key + ":blocks"])
    slots = d[key + ":slots"]
    pos = np.frombuffer(d[key + ":pos"].tobytes(), dtype=features.features_dtype()).copy()
    n, D = len(pos), dm // heads
    for stop in range(nblk + 1):
        os.environ["P3HIP_DEBUG_STOP_BLOCK"] = str(stop)
        eng = engine.HipEngine(path, n)
        eng.load_all(pos)
        eng.RunInference()
        x = eng.debug_x(n, Cs)
        out[f"{key}:x{stop}"] = x[slots].astype(np.float16)
        out[f"{key}:xpad{stop}"] = np.array(bool((x[:, dm:] == 0).all()) and bool(np.isfinite(x).all()))
        if stop > 0:
            for w, t in enumerate("qkvo"):
                a = eng.debug_tfm(w, n, heads, D)
                out[f"{key}:{t}{stop - 1}"] = a[slots].astype(np.float16)
                if w < 3:
                    out[f"{key}:{t}pad{stop - 1}"] = np.array(bool((a[:, :, 361:] == 0).all()) and bool(np.isfinite(a).all()))
                else:
                    out[f"{key}:ofinite{stop - 1}"] = np.array(bool(np.isfinite(a).all()))
        if stop == nblk:
            few = max(1, n // 3)
            for s in range(few):                 # a second run with fewer slots loaded: compacted to `few` positions
                eng.LoadBatch(s, pos[n - 1 - s:n - s])
            eng.RunInference()
            out[f"{key}:pad_compact"] = np.array(zero_rows(eng, few, heads, D))
            eng.load_all(pos)                    # and a third with all of them
            eng.RunInference()
            out[f"{key}:pad_again"] = np.array(zero_rows(eng, n, heads, D))
            again = eng.debug_tfm(3, n, heads, D)[slots].astype(np.float16)
            out[f"{key}:o_again"] = np.array(bool(np.array_equal(again, out[f"{key}:o{nblk - 1}"])))
        eng.close()
    os.environ.pop("P3HIP_DEBUG_STOP_BLOCK", None)
    eng = engine.HipEngine(path, n)              # the whole pass, heads included
    eng.load_all(pos)
    eng.RunInference()
    out[f"{key}:raw"] = np.stack([eng.get_raw(int(s)) for s in slots])
    out[f"{key}:xfull"] = eng.debug_x(n, Cs)[slots].astype(np.float16)
    eng.close()
np.savez(sys.argv[2], **out)
"""


def _weights(name):
    """(cfg, weights of the emulation, weights the engine gets) of a job name `net[:hot|:m1]`."""
    net, _, var = name.partition(":")
    cfg, W = T.hot_weights(net) if var == "hot" else dh.fixture_weights(net)
    Weng = W
    if var == "m1":
        Weng = dict(W)
        key = f"blocks.{M1['block']}.k.w"
        D = cfg.channels // cfg.bottleneck_channels
        a, b = (M1["head"] * D + l for l in M1["lanes"])
        w = W[key].copy()
        w[:, [a, b]] = w[:, [b, a]]
        Weng[key] = w
    return cfg, W, Weng


def _run_child(tmp_path, jobs, label):
    from p3achygo_amd import netspec
    spec = {"keys": np.array([j[0] for j in jobs])}
    meta = {}
    for name, batch in jobs:
        cfg, W, Weng = _weights(name)
        path = str(tmp_path / (name.replace(":", "_") + ".p3w"))
        netspec.save_p3w(path, cfg, Weng)
        pos, slots, gslots = _batch(name, batch)
        d = cfg.channels
        spec.update({name + ":path": np.array(path), name + ":d": np.array(d),
                     name + ":Cs": np.array(128 if d <= 128 else (256 if d <= 256 else 384)),
                     name + ":heads": np.array(cfg.bottleneck_channels), name + ":blocks": np.array(cfg.blocks),
                     name + ":slots": slots, name + ":pos": np.frombuffer(pos.tobytes(), np.uint8)})
        meta[name] = (cfg, W, pos, slots, gslots)
    inp, outp = tmp_path / f"{label}_in.npz", tmp_path / f"{label}_out.npz"
    np.savez(inp, **spec)
    env = dict(os.environ)
    env.pop("P3HIP_DEBUG_STOP_BLOCK", None)
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, str(inp), str(outp)], env=env, capture_output=True,
                       text=True, timeout=CHILD_LIMITS[label])
    print(f"{label} child: {time.time() - t0:.0f} s")
    assert r.returncode == 0, r.stderr[-3000:]
    return meta, np.load(outp)


def _record(out, name, cfg):
    """The engine's tensors of one job in tfm_emulation's layouts."""
    d, nb = cfg.channels, cfg.blocks
    rec = {"x": [T.tokens(out[f"{name}:x{s}"], d) for s in range(nb + 1)]}
    for t in "qkv":
        rec[t] = [np.asarray(out[f"{name}:{t}{i}"], np.float64)[:, :, :T.L] for i in range(nb)]
    rec["o"] = [np.asarray(out[f"{name}:o{i}"], np.float64) for i in range(nb)]
    return rec


def _invariants(out, name, cfg):
    for s in range(cfg.blocks + 1):
        assert bool(out[f"{name}:xpad{s}"]), f"{name}: padding channels of x not zero, or x not finite, in front of block {s}"
    for i in range(cfg.blocks):
        for t in "qkv":
            assert bool(out[f"{name}:{t}pad{i}"]), f"{name}: rows 361..383 of {t} not zero, or {t} not finite, after block {i}"
        assert bool(out[f"{name}:ofinite{i}"]), f"{name}: o of block {i} not finite"
    assert bool(out[f"{name}:pad_compact"]), f"{name}: rows 361..383 of q, k, v not zero after a run with fewer slots"
    assert bool(out[f"{name}:pad_again"]), f"{name}: rows 361..383 of q, k, v not zero after the third run"
    assert bool(out[f"{name}:o_again"]), f"{name}: o of the last block differs between the first and the third run"
    # the stopped engine computed what the whole pass computes
    assert np.array_equal(out[f"{name}:xfull"], out[f"{name}:x{cfg.blocks}"]), f"{name}: stopped and whole pass differ in x"


def _judge(jobs, meta, out):
    fam: dict = {}
    for name, _ in jobs:
        cfg, W, pos, slots, gslots = meta[name]
        rec = _record(out, name, cfg)
        emu = T.Tfm(cfg, W)
        _invariants(out, name, cfg)
        if name.endswith(":m1"):
            with pytest.raises(AssertionError) as exc:
                T.teacher_forced(emu, rec, pos[slots], slots=slots, label=f"{name} block ")
            msg = str(exc.value)
            print(msg)
            assert msg.startswith(f"block {name} block {M1['block']} k_tfm_qkv k:"), msg
            assert f"heads over the bound [{M1['head']}]" in msg, msg
            _report_m1(name, out[f"{name}:raw"], slots, gslots)
            continue
        hot = name.endswith(":hot")
        if hot:
            x = max(float(np.abs(np.asarray(a)).max()) for a in rec["x"])
            reg = T.attention_regime(emu, rec["q"][0], rec["k"][0])
            print(f"{name}: engine max |x| {x:.1f}, block 0 of the engine's q, k: " +
                  ", ".join(f"{k} {v:.3f}" for k, v in reg.items()))
            assert x < 4096 and reg["peak"] >= 0.7 and reg["tiny"] >= 0.8
        st = T.teacher_forced(emu, rec, pos[slots], slots=slots, label=f"{name} block ", hot=hot)
        T.collect(fam, cfg, st, hot)
    for f, (ident, err) in sorted(fam.items()):
        print(f"{f}: lowest fraction identical {ident:.3f}, max err {err:.2f}")


def _report_m1(name, raw, slots, gslots):
    """Information only: would the output-level bounds of test_transformer_gpu.py have flagged the exchanged channels?"""
    from test_transformer_gpu import LOGIT_REL, TOL
    net = name.partition(":")[0]
    g, _ = load_golden(net)
    flagged = []
    for k, s in enumerate(gslots):
        got, want = raw[list(slots).index(s)], g["raw"][k]
        flagged.append(not (np.abs(got - want) <= np.maximum(TOL[net]["logit"], LOGIT_REL * np.abs(want))).all())
        print(f"M1 replay, fixture position {k}: max |d| of the raw outputs {np.abs(got - want).max():.2e} "
              f"(bound {TOL[net]['logit']:.2e})")
    print(f"M1 replay: the output-level bounds would {'' if any(flagged) else 'NOT '}have flagged it")


def test_kernels_teacher_forced(built, tmp_path):
    """Every kernel of every block of the eight fixture nets, and the stem, from the engine's own input, inside
    tfm_emulation.BOUNDS; the padding rows and channels exactly zero."""
    meta, out = _run_child(tmp_path, PLAIN_JOBS, "plain")
    _judge(PLAIN_JOBS, meta, out)


def test_kernels_teacher_forced_peaked_attention(built, tmp_path):
    """The same with Wq, Wk x 4 (most softmax numerators below fp16's range, the online softmax really rescaling), and
    the :m1 job, which must be rejected at k_tfm_qkv of block 1 and nowhere earlier."""
    meta, out = _run_child(tmp_path, HOT_JOBS, "hot")
    _judge(HOT_JOBS, meta, out)


def test_debug_tfm_refuses_what_it_cannot_answer(built, tmp_path, weight_files):
    """p3hip_debug_tfm: non-zero for a conv engine, for another `which`, and for more positions than the last run had."""
    from p3achygo_amd import engine, netspec
    cfg, W, _ = _weights("test_b2d64h2_tfm")
    path = str(tmp_path / "t.p3w")
    netspec.save_p3w(path, cfg, W)
    _, pos = load_golden("test_b2d64h2_tfm")
    eng = engine.HipEngine(path, 8)
    with pytest.raises(engine.EngineError):
        eng.debug_tfm(0, 1, 2, 32)               # nothing has run yet
    for s in range(3):
        eng.LoadBatch(s, pos[s:s + 1])
    eng.RunInference()
    assert eng.debug_tfm(0, 3, 2, 32).shape == (3, 2, 384, 32) and eng.debug_tfm(3, 3, 2, 32).shape == (3, 361, 64)
    for which, n in ((0, 4), (4, 1), (-1, 1), (1, 0)):
        with pytest.raises(engine.EngineError):
            eng.debug_tfm(which, n, 2, 32)
    eng.close()
    conv = engine.HipEngine(weight_files("test_b3c128btl2"), 2)
    conv.load_all(pos[:2])
    conv.RunInference()
    with pytest.raises(engine.EngineError):
        conv.debug_tfm(0, 1, 2, 32)
    conv.close()
