"""The conv trunks block by block against the fp16 emulation (tests/trunk_emulation.py), with teacher forcing: the
emulation of block k starts from the engine's own x after block k - 1 (P3HIP_DEBUG_STOP_BLOCK, read per engine at
create, with p3hip_debug_x), so errors do not cascade and every block, the stem and the heads are judged on their own
by trunk_emulation.check_block, whose thresholds the twin sets on the CPU (tests/test_trunk_emulation_cpu.py).

Each GPU configuration runs in one child process under its own time limit; a failing child fails the test, nothing
retries.  The block child sets P3HIP_NO_FUSE=1 P3HIP_NO_BFUSE=1, so that every block boundary is a stop point;
test_fused_block_launches_equal_one_launch_per_block (test_engine_gpu.py) ties the fused launches bit for bit to it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import trunk_emulation as te  # noqa: E402
from conftest import ROOT, load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

# (net, batch): the 11 test nets and b12c256btl3 — C = 128, 192, 256, 384; btl, nbt, classic, _i2 and broadcast blocks;
# fused and layer-wise trunks — at batches of 1, 37 and 300 (more positions than CUs: workgroups take several)
BLOCK_JOBS = [("test_b3c128btl2", 37), ("test_b3c128nbt", 300), ("test_b3c256btl1", 1), ("test_b3c256nbt", 37),
              ("test_b3c384btl3", 37), ("test_b3c384nbt", 300), ("test_b3c192classic", 37), ("test_b5c256nbt_i2", 37),
              ("test_b5c128btl1_i2", 37), ("test_b5c256btl2_i2", 300), ("test_b10c256btl1_i2", 37), ("b12c256btl3", 300),
              ("test_b3c256btl1:hot", 37), ("test_b3c384nbt:hot", 37), ("test_b3c256btl1:m1", 37)]
HEAD_JOBS = [("test_b3c256btl1", 37), ("b12c256btl3", 300), ("test_b3c384nbt", 37)]   # k_headsx, k_headsx, k_heads
M1 = dict(kind="M1", block=0, conv=1, channel=37)

_CHILD = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np
from p3achygo_amd import engine, features
d = np.load(sys.argv[1], allow_pickle=True)
out = {}
for key in d["keys"]:
    path, C, nblk, slots, stops = d[key + ":path"].item(), int(d[key + ":C"]), int(d[key + ":blocks"]), d[key + ":slots"], d[key + ":stops"]
    pos = np.frombuffer(d[key + ":pos"].tobytes(), dtype=features.features_dtype()).copy()
    for stop in stops:
        if stop < nblk:
            os.environ["P3HIP_DEBUG_STOP_BLOCK"] = str(stop)
        else:
            os.environ.pop("P3HIP_DEBUG_STOP_BLOCK", None)
        eng = engine.HipEngine(path, len(pos))
        eng.load_all(pos)
        eng.RunInference()
        out[f"{key}:x{stop}"] = eng.debug_x(len(pos), C)[slots]
        if stop == nblk:
            out[f"{key}:raw"] = np.stack([eng.get_raw(int(s)) for s in slots])
        eng.close()
np.savez(sys.argv[2], **out)
"""


def _weights(name):
    """(cfg, fixture weights, weights the engine gets) of a job name `net[:hot|:m1]`; hot: trunk_emulation.hot_weights
    calibrated on the net's golden positions."""
    from p3achygo_amd import netspec
    net, _, var = name.partition(":")
    cfg = netspec.CONFIGS[net]
    W = netspec.generate_weights(cfg, randomize=True)
    if var == "hot":
        W = te.hot_weights(cfg, W, load_golden(net)[1])
    Weng = W
    if var == "m1":
        Weng = dict(W)
        k = f"blocks.{M1['block']}.conv{M1['conv']}.w"
        Weng[k] = W[k].copy()
        Weng[k][:, :, :, M1["channel"]] = W[k][:, ::-1, :, M1["channel"]]   # HWIO: mirror the columns
    return cfg, W, Weng


def handmade_positions():
    """An empty board with no moves, a crowded board with captures, komi of both signs and large magnitude, and a
    pass-heavy history."""
    from p3achygo_amd import features
    pos = features.random_positions(6, seed=77, min_moves=330, max_moves=420, n_games=6, pass_prob=0.02)
    for key in ("board", "stones_atari", "stones_two_liberties", "stones_three_liberties", "stones_laddered"):
        pos[0][key] = 0
    pos[0]["last_moves"]["i"], pos[0]["last_moves"]["j"] = -1, -1
    pos[0]["komi"] = 7.5
    pos[2]["komi"], pos[3]["komi"] = -150.0, 150.0
    pos[4]["last_moves"]["i"], pos[4]["last_moves"]["j"] = 19, 0
    pos[5]["komi"] = -0.5
    return pos


def _batch(name, batch):
    """Positions of a job: the fixture's and the hand-made ones scattered among seeded fill; the compared slots: those,
    a strided sample and the last one."""
    from p3achygo_amd import features
    net = name.partition(":")[0]
    _, gpos = load_golden(net)
    special = np.concatenate([gpos, handmade_positions()])[:batch]
    pos = features.random_positions(batch, seed=43, n_games=16, max_moves=300, komis=(7.5, -7.5, 0.5))
    at = [int(s) for s in np.linspace(0, batch - 1, len(special)).round()] if batch > 1 else [0]
    pos[at] = special[:len(at)]
    slots = sorted(set(at) | set(range(5, batch, 29)) | {batch - 1})
    return pos, np.asarray(slots), at[:len(gpos)]


def _run_child(tmp_path, jobs, env_extra, label, timeout):
    from p3achygo_amd import netspec
    spec = {"keys": np.array([j[0] for j in jobs])}
    meta = {}
    for name, batch, stops in jobs:
        cfg, W, Weng = _weights(name)
        path = str(tmp_path / (name.replace(":", "_") + ".p3w"))
        netspec.save_p3w(path, cfg, Weng)
        pos, slots, gslots = _batch(name, batch)
        spec.update({name + ":path": np.array(path), name + ":C": np.array(cfg.channels),
                     name + ":blocks": np.array(cfg.blocks), name + ":slots": slots, name + ":stops": np.asarray(stops),
                     name + ":pos": np.frombuffer(pos.tobytes(), np.uint8)})
        meta[name] = (cfg, W, pos, slots, gslots)
    inp, outp = tmp_path / f"{label}_in.npz", tmp_path / f"{label}_out.npz"
    np.savez(inp, **spec)
    env = dict(os.environ)
    for k in ("P3HIP_NO_FUSE", "P3HIP_NO_BFUSE", "P3HIP_DEBUG_STOP_BLOCK"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, str(inp), str(outp)], env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return meta, np.load(outp)


def test_blocks_teacher_forced(built, tmp_path):
    """Every block of every net, and the stem, from the engine's own input, inside trunk_emulation's bounds."""
    from p3achygo_amd import netspec
    jobs = [(n, b, list(range(netspec.CONFIGS[n.partition(":")[0]].blocks + 1))) for n, b in BLOCK_JOBS]
    meta, out = _run_child(tmp_path, jobs, {"P3HIP_NO_FUSE": "1", "P3HIP_NO_BFUSE": "1"}, "blocks", 600)
    fam: dict = {}
    for name, _, stops in jobs:
        cfg, W, pos, slots, gslots = meta[name]
        xs = [out[f"{name}:x{s}"] for s in stops]
        emu = te.Trunk(cfg, W)
        if name.endswith(":m1"):
            with pytest.raises(AssertionError) as exc:
                te.teacher_forced(emu, xs, pos[slots], slots=slots, label=f"{name} block ")
            assert f"{name} block {M1['block']} " in str(exc.value), str(exc.value)
            _report_m1(name, out[f"{name}:raw"], slots, gslots)
            continue
        hot = name.endswith(":hot")
        if hot:   # large fp16 ulps and mish's asymptotes, not inf or NaN
            top = max(float(x.abs().max()) for x in te.Trunk(cfg, W).trunk(pos[slots]))
            print(f"{name}: emulated max |x| {top:.0f}")
            assert 100 < top < 4096
        st = te.teacher_forced(emu, xs, pos[slots], slots=slots, label=f"{name} block ", hot=hot)
        for k, s in st.items():
            f = "stem" if k == "stem" else f"C{cfg.channels} {cfg.block_kind(k)}" + (" hot" if hot else "")
            a = fam.setdefault(f, [1.0, 0.0])
            a[0], a[1] = min(a[0], s["identical"]), max(a[1], s["max_err"])
    for f, (ident, err) in sorted(fam.items()):
        print(f"{f}: lowest fraction identical {ident:.3f}, max err {err:.2f}")


def _report_m1(name, raw, slots, gslots):
    """Information only: would the output-level bounds of test_engine_gpu.py have flagged the mirrored kernel?"""
    from test_engine_gpu import LOGIT_TOL, _logits_close
    g, _ = load_golden(name.partition(":")[0])
    flagged = []
    for k, s in enumerate(gslots):
        got = raw[list(slots).index(s)]
        flagged.append(not (_logits_close(got[:1887], g["raw"][k][:1887]) and
                            np.abs(got[1887:] - g["raw"][k][1887:]).max() <= LOGIT_TOL))
        print(f"M1 replay, fixture position {k}: max |d| of the raw outputs {np.abs(got - g['raw'][k]).max():.2e}")
    print(f"M1 replay: the output-level bounds would {'' if any(flagged) else 'NOT '}have flagged it")


def test_heads_on_the_engines_own_trunk_output(built, tmp_path):
    """The shipping configuration (fused, joined blocks; k_headsx, or k_heads at C = 384): get_raw against heads() in
    float64 on the engine's own x."""
    from p3achygo_amd import netspec
    jobs = [(n, b, [netspec.CONFIGS[n].blocks]) for n, b in HEAD_JOBS]
    meta, out = _run_child(tmp_path, jobs, {}, "heads", 300)
    for name, _, stops in jobs:
        cfg, W, pos, slots, _ = meta[name]
        x = out[f"{name}:x{stops[0]}"].reshape(len(slots), cfg.channels, 19, 19)
        import torch
        want = te.Trunk(cfg, W).heads(torch.from_numpy(x.astype(np.float64)))
        d = np.abs(out[f"{name}:raw"] - want)
        print(f"{name} heads: max |d| {d.max():.2e}")
        assert d.max() <= te.HEADS_TOL, (name, np.unravel_index(int(d.argmax()), d.shape))
