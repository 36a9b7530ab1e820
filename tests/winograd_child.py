"""The child process of tests/test_winograd_gpu.py: every step that creates more than one engine runs here, one engine at a
time, and leaves arrays for the parent to judge.

    python tests/winograd_child.py JOB IN.npz OUT.npz

JOB blocks: IN path, Cp, blocks, batches -> per batch b: "b<b>:x<stop>" (the stream in front of block stop, stop = blocks:
    behind the last), "b<b>:raw", "b<b>:x0_fp16" (the fp16 engine's stem), all at the slots of
    test_conv_widths_gpu.block_batch.
JOB forms: IN keys, paths, flags -> "<key>:raw" at batch 37, "<key>:kernel", "<key>:flops", "<key>:ms" (the timing hook).
JOB mech: IN path, garbage (a .p3w or ""), -> the composition battery on one net, see the code.

TEST INFRASTRUCTURE ONLY."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402


def _run(eng, pos, slots=None):
    slots = list(range(len(pos))) if slots is None else slots
    for k, s in enumerate(slots):
        eng.LoadBatch(s, pos[k:k + 1])
    eng.RunInference()
    return np.stack([eng.get_raw(s) for s in slots])


def blocks(engine, d, out):
    from test_conv_widths_gpu import block_batch
    path, Cp, nblk = d["path"].item(), int(d["Cp"]), int(d["blocks"])
    for batch in [int(b) for b in d["batches"]]:
        pos, slots = block_batch(batch)
        for stop in range(nblk + 1):
            os.environ["P3HIP_DEBUG_STOP_BLOCK"] = str(stop)   # (stop = nblk: in front of the heads)
            if stop == nblk:
                os.environ.pop("P3HIP_DEBUG_STOP_BLOCK")
            eng = engine.HipEngine(path, batch, flags=engine.FLAG_WINOGRAD)
            eng.load_all(pos)
            eng.RunInference()
            out["b%d:x%d" % (batch, stop)] = eng.debug_x(batch, Cp)[slots]
            if stop == nblk:
                out["b%d:raw" % batch] = np.stack([eng.get_raw(int(s)) for s in slots])
            eng.close()
        os.environ["P3HIP_DEBUG_STOP_BLOCK"] = "0"
        eng = engine.HipEngine(path, batch)
        eng.load_all(pos)
        eng.RunInference()
        out["b%d:x0_fp16" % batch] = eng.debug_x(batch, Cp)[slots]
        eng.close()
        os.environ.pop("P3HIP_DEBUG_STOP_BLOCK")


def forms(engine, d, out):
    from p3achygo_amd import features
    pos = features.random_positions(37, seed=43)
    for key, path, flag in zip(d["keys"], d["paths"], d["flags"]):
        eng = engine.HipEngine(str(path), 37, flags=int(flag))
        out[key + ":raw"] = _run(eng, pos)
        ms, fl, kname = eng.time_trunk_kernel(37, 1)
        out[key + ":kernel"], out[key + ":flops"], out[key + ":ms"] = np.array(kname), np.array(fl), np.array(ms)
        eng.close()


def mech(engine, d, out):
    from p3achygo_amd import features
    path, F = d["path"].item(), engine.FLAG_WINOGRAD
    # copies of a position at rows 0-31 and 96-127 of a batch of 128; three runs on two engines
    pos = np.tile(features.random_positions(32, seed=2, n_games=8), 4).copy()
    k = 0
    for _ in range(2):
        eng = engine.HipEngine(path, 128, flags=F)
        for _ in range(3):
            eng.load_all(pos)
            eng.RunInference()
            out["repeat:%d" % k] = np.stack([eng.get_raw(s) for s in range(128)])
            k += 1
        eng.close()
    # 20 of 64 slots compacted, RUN_ALL_SLOTS
    pos = features.random_positions(20, seed=17)
    slots = list(range(2, 62, 3))
    for key, batch, fl, sl in (("plain20", 20, 0, None), ("compact", 64, 0, slots), ("allslots", 64, engine.FLAG_RUN_ALL_SLOTS, slots)):
        eng = engine.HipEngine(path, batch, flags=F | fl)
        out[key] = _run(eng, pos, sl)
        eng.close()
    # graph replay: eager, capture, replay, replay
    pos = features.random_positions(32, seed=8)
    eng = engine.HipEngine(path, 32, flags=F)
    out["graph:want"] = _run(eng, pos)
    eng.close()
    eng = engine.HipEngine(path, 32, flags=F | engine.FLAG_LAUNCH_GRAPH)
    for rnd in range(4):
        out["graph:%d" % rnd] = _run(eng, pos)
    out["graph:state"] = np.array(eng.graph_state())
    eng.close()
    # NN-cache hits; AUX on top
    pos = features.random_positions(16, seed=12)
    eng = engine.HipEngine(path, 16, flags=F)
    out["plain16"] = _run(eng, pos)
    out["plain16:rec"] = np.stack([np.ctypeslib.as_array(eng.GetBatch(s).move_probs).copy() for s in range(16)])
    eng.close()
    eng = engine.HipEngine(path, 16, flags=F)
    eng.EnableCache(8)
    for rnd in range(2):
        for i in range(16):
            eng.LoadBatchKeyed(i, pos[i:i + 1], 1000 + i, 77)
        eng.RunInference()
        res = [eng.GetBatchKeyed(i) for i in range(16)]
        out["cache:%d:hit" % rnd] = np.array([h for _, _, h in res])
        out["cache:%d:logits" % rnd] = np.stack([np.ctypeslib.as_array(r.move_logits).copy() for r, _, _ in res])
    eng.close()
    eng = engine.HipEngine(path, 16, flags=F | engine.FLAG_AUX)
    out["aux:raw"] = _run(eng, pos)
    out["aux:rec"] = np.stack([np.ctypeslib.as_array(eng.GetBatch(s).move_probs).copy() for s in range(16)])
    out["aux:aux"] = np.stack([eng.GetAux(s) for s in range(16)])
    eng.close()
    # poison in front of a full and a five-row run
    for mode, byte in (("clean", None), ("ff", 0xFF), ("7b", 0x7B)):
        eng = engine.HipEngine(path, 16, flags=F)
        for n in (16, 5):
            if byte is not None:
                eng.debug_poison(byte)
            out["poison:%s:%d" % (mode, n)] = _run(eng, pos[:n])
        eng.close()
    # garbage in the padded weight channels
    pos = features.random_positions(37, seed=43)
    for key in ("pad", "garbage"):
        eng = engine.HipEngine(d[key].item(), 37, flags=F)
        out["twin:" + key] = _run(eng, pos)
        eng.close()


if __name__ == "__main__":
    from p3achygo_amd import engine
    job, inp, outp = sys.argv[1:4]
    res = {}
    {"blocks": blocks, "forms": forms, "mech": mech}[job](engine, np.load(inp, allow_pickle=True), res)
    np.savez(outp, **res)
