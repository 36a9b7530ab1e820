"""A captured graph for runs of every size (P3HIP_FLAG_LAUNCH_GRAPH_ANY) against
P3HIP_FLAG_LAUNCH_GRAPH alone, interleaved A/B on one MI355X.  Every figure is the wall time of p3hip_run alone: the
slots are loaded outside the timed call.  A leg is 200 runs; the legs of a case alternate, three rounds each; a case's
summary has the median of each leg's round means and its spread (max / min over the rounds).

Blocks (--blocks, default all five):
  partial  the low-latency plans (P3HIP_FLAG_LOW_LATENCY_ANY) with fewer slots loaded than the engine has: an engine of
           8 slots with 1, 3 and 7 loaded, one of 32 with 5 and 20, on four nets.  Legs: graph (LAUNCH_GRAPH alone: every
           such run goes out kernel by kernel), any (the new flag: every size replays its own graph).
  worst    the worst case for the table: b12c256btl3 at 1024 slots with the NN cache on and a miss count drawn uniformly
           from 1..1024 per run (the hits are keys stored before, the misses unkeyed slots), so almost every key is new
           and a capture can only cost.  Legs: graph, any, and any under the settings named by --worst-variants
           (P3HIP_GRAPH_MIN_SEEN / P3HIP_GRAPH_MAX_ROWS in the environment of the leg's p3hip_create).
  symslot  P3HIP_FLAG_SYMMETRY_SLOT on b12c256btl3: one root at 0xFF and 1023 leaves, 1031 forward rows.  Legs: graph, any.
  parent   (--parent-lib) the unflagged engine and the LAUNCH_GRAPH engine of this build against the same two of the parent
           commit's library, b12c256btl3 at 1024 slots, all loaded.  A process holds one build, so the builds alternate as
           child processes.
  match    an eval match of one game with eight search threads per game, both players on the low-latency plan with the
           new flag (nn_low_latency: 1, nn_graph_any: 1): the engines' p3hip_graph_stats summed at the end.

  python tools/gpu_graph_any_ab.py --out profiles/graph_any_ab.jsonl [--parent-lib PARENT/p3achygo_amd/csrc/libp3hip.so]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTIAL_NETS = ["b12c256btl3", "b14c384btl3", "b12c128btl3", "b14d96h3_transformer"]
PARTIAL_CASES = [(8, 1), (8, 3), (8, 7), (32, 5), (32, 20)]
BIG = "b12c256btl3"
RUNS, ROUNDS = 200, 3

_weights = {}


def weights(name, d):
    from p3achygo_amd import netspec
    if name not in _weights:
        cfg = netspec.get_config(name)
        _weights[name] = os.path.join(d, name + ".p3w")
        netspec.save_p3w(_weights[name], cfg, netspec.generate_weights(cfg, randomize=True))
    return _weights[name]


def create(path, batch, flags, env=None, **kw):
    """an engine created under `env` (the P3HIP_* switches are read at p3hip_create)"""
    from p3achygo_amd import engine
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return engine.HipEngine(path, batch, flags=flags, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def time_leg(eng, load, runs, fetch=None):
    """ms of each of `runs` p3hip_run calls; load(i) before and fetch() after every run stay outside the clock"""
    from p3achygo_amd.power_sampler import PowerSampler
    try:
        sampler = PowerSampler(0)
        sampler.start()
    except Exception:
        sampler = None
    ms = np.zeros(runs)
    for i in range(runs):
        load(i)
        t0 = time.perf_counter()
        eng.RunInference()
        ms[i] = (time.perf_counter() - t0) * 1e3
        if fetch:
            fetch()
    return {"run_ms": float(ms.mean()), "run_ms_p50": float(np.median(ms)), "run_ms_max": float(ms.max()), "runs": runs,
            "chip": sampler.stop() if sampler else None}


def stats_of(eng):
    from p3achygo_amd import engine
    try:
        return eng.graph_stats()
    except (engine.EngineError, AttributeError):   # no graph flag; the parent commit's library has no such function
        return None


def run_case(tag, legs, emit, rounds=ROUNDS, runs=RUNS, warm=4):
    """legs: name -> (engine, load, fetch).  Warm-up: `warm` runs of every leg over the loads of the timed runs' first ones"""
    for eng, load, fetch in legs.values():
        for i in range(warm):
            load(i)
            eng.RunInference()
            if fetch:
                fetch()
    res = {k: [] for k in legs}
    for r in range(rounds):
        for name, (eng, load, fetch) in legs.items():
            x = time_leg(eng, load, runs, fetch)
            x.update(tag)
            x.update({"leg": name, "round": r, "graph_stats": stats_of(eng), "graph_state": eng.graph_state()})
            emit(x)
            res[name].append(x["run_ms"])
    s = dict(tag)
    s["summary"] = True
    for name, v in res.items():
        v = sorted(v)
        s[name + "_run_ms"] = v[len(v) // 2]
        s[name + "_spread"] = v[-1] / v[0]
    base = s.get("graph_run_ms")
    for name in res:
        if base and name != "graph":
            s[name + "_over_graph"] = s[name + "_run_ms"] / base
    emit(s)
    for eng, _, _ in legs.values():
        eng.close()
    return s


def block_partial(d, emit, nets):
    from p3achygo_amd import engine, features
    LL = engine.FLAG_LOW_LATENCY_ANY
    for name in nets:
        path = weights(name, d)
        for batch, n in PARTIAL_CASES:
            pos = features.random_positions(batch, seed=7, n_games=4)
            legs = {}
            for leg, flags in (("graph", LL | engine.FLAG_LAUNCH_GRAPH), ("any", LL | engine.FLAG_LAUNCH_GRAPH_ANY)):
                eng = create(path, batch, flags)

                def load(i, eng=eng):
                    for s in range(n):
                        eng.LoadBatch(s, pos[(s + i) % batch:(s + i) % batch + 1])

                def fetch(eng=eng):
                    for s in range(n):
                        eng.GetBatch(s)
                legs[leg] = (eng, load, fetch)
            run_case({"block": "partial", "net": name, "batch": batch, "loaded": n}, legs, emit)


def block_worst(d, emit, variants):
    """the miss count of run i is the same in every leg; a slot's result is fetched after the run, or it would stay in the
    next one"""
    from p3achygo_amd import engine, features
    batch = 1024
    path = weights(BIG, d)
    pos = features.random_positions(batch, seed=9, n_games=64)
    sz = pos.dtype.itemsize
    counts = np.random.default_rng(5).integers(1, batch + 1, size=4 + ROUNDS * RUNS)
    keys = [((0x9E3779B97F4A7C15 * (s + 1)) & (2**64 - 1), (0xC2B2AE3D27D4EB4F * (s + 7)) & (2**64 - 1)) for s in range(batch)]
    key = lambda s: keys[s]
    legs = {}
    specs = [("graph", engine.FLAG_LAUNCH_GRAPH, {}), ("any", engine.FLAG_LAUNCH_GRAPH_ANY, {})]
    for v in variants:
        env = dict(kv.split("=") for kv in v.split(","))
        specs.append(("any_" + v.replace("P3HIP_GRAPH_", "").lower(), engine.FLAG_LAUNCH_GRAPH_ANY, env))
    for leg, flags, env in specs:
        eng = create(path, batch, flags, env)
        eng.EnableCache(14)
        L, h = eng._L, eng._h
        for s in range(batch):                                   # every slot's key into the table
            eng.LoadBatchKeyed(s, pos[s:s + 1], *key(s))
        eng.RunInference()
        res = engine.Result()
        state = {"at": 0}

        def load(i, eng=eng, L=L, h=h, state=state):
            m = int(counts[state["at"] % len(counts)])
            state["at"] += 1
            base = pos.ctypes.data
            for s in range(m):                                   # unkeyed: a miss, never stored
                L.p3hip_load_slot(h, s, base + s * sz)
            for s in range(m, batch):
                L.p3hip_load_slot_keyed(h, s, base + s * sz, *key(s), 0)

        def fetch(L=L, h=h, res=res):
            import ctypes as C
            for s in range(batch):
                L.p3hip_get_slot(h, s, C.addressof(res))
        fetch()
        legs[leg] = (eng, load, fetch)
    # (every leg's loads are called equally often, so round r of every leg draws the same 200 counts)
    return run_case({"block": "worst", "net": BIG, "batch": batch, "cache": True}, legs, emit)


def block_symslot(d, emit):
    from p3achygo_amd import engine, features
    batch = 1024
    path = weights(BIG, d)
    pos = features.random_positions(batch, seed=7, n_games=64)
    syms = np.random.default_rng(11).integers(0, 8, batch)
    masks = [1 << int(s) for s in syms]
    masks[0] = 0xFF
    legs = {}
    for leg, g in (("graph", engine.FLAG_LAUNCH_GRAPH), ("any", engine.FLAG_LAUNCH_GRAPH_ANY)):
        eng = create(path, batch, engine.FLAG_SYMMETRY_SLOT | g, symmetry_rows=batch + 7)

        def load(i, eng=eng):
            eng.load_all(pos)
            for s, m in enumerate(masks):
                eng.set_slot_symmetries(s, m)
        legs[leg] = (eng, load, None)
    run_case({"block": "symslot", "net": BIG, "batch": batch, "rows": batch + 7}, legs, emit, runs=100)


def block_parent_child(d, emit, build):
    """one round of the two legs on whatever library P3HIP_LIB names"""
    from p3achygo_amd import engine, features
    batch = 1024
    path = weights(BIG, d)
    pos = features.random_positions(batch, seed=7, n_games=64)
    legs = {}
    for leg, flags in (("plain", 0), ("graph", engine.FLAG_LAUNCH_GRAPH)):
        eng = create(path, batch, flags)
        legs[leg] = (eng, lambda i, eng=eng: eng.load_all(pos), None)
    run_case({"block": "parent", "net": BIG, "batch": batch, "build": build}, legs, emit, rounds=1, runs=100)


def block_match(d, emit):
    from p3achygo_amd import host_api
    path = weights("b12c128btl3", d)
    flags = "nn_low_latency: 1\nnn_graph_any: 1\n"
    host_api.eval_set_player_flags(flags, flags)
    host_api.graph_stats()
    try:
        t0 = time.perf_counter()
        st = host_api.eval_match_threads(path, path, num_games=1, visits_per_move=96, threads_per_game=8, max_moves=60,
                                         cache_size=1 << 14, seed=3)
        secs = time.perf_counter() - t0
    finally:
        host_api.eval_set_player_flags("", "")
    emit({"block": "match", "net": "b12c128btl3", "threads_per_game": 8, "games": 1, "moves": st.moves, "batches": st.batches,
          "positions": st.positions, "seconds": secs, "graph_stats_both_players": host_api.graph_stats()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", nargs="*", default=["partial", "worst", "symslot", "parent", "match"])
    ap.add_argument("--nets", nargs="*", default=PARTIAL_NETS)
    ap.add_argument("--worst-variants", nargs="*", default=[],
                    help="settings of further `any` legs of the worst case, e.g. P3HIP_GRAPH_MIN_SEEN=3 P3HIP_GRAPH_MAX_ROWS=256")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()

    def emit(x):
        print(json.dumps(x), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(x) + "\n")

    with tempfile.TemporaryDirectory() as d:
        if args.parent_child:
            return block_parent_child(d, emit, args.parent_child)
        if "partial" in args.blocks:
            block_partial(d, emit, args.nets)
        if "worst" in args.blocks:
            block_worst(d, emit, args.worst_variants)
        if "symslot" in args.blocks:
            block_symslot(d, emit)
        if "match" in args.blocks:
            block_match(d, emit)
    if "parent" in args.blocks and args.parent_lib:
        rows = []
        for r in range(ROUNDS):
            for build, lib in (("this commit", None), ("parent commit", os.path.abspath(args.parent_lib))):
                env = dict(os.environ)
                if lib:
                    env["P3HIP_LIB"] = lib
                cmd = [sys.executable, os.path.abspath(__file__), "--parent-child", build]
                out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
                if out.returncode != 0:
                    sys.exit(f"the {build} leg failed with exit status {out.returncode}: {out.stderr[-2000:]}")
                for ln in out.stdout.splitlines():
                    if not ln.startswith("{"):
                        continue
                    x = json.loads(ln)
                    if not x.get("summary"):
                        x["round"] = r
                        emit(x)
                        rows.append(x)
        s = {"summary": True, "block": "parent", "net": BIG, "batch": 1024}
        for build, k in (("this commit", "this"), ("parent commit", "parent")):
            for leg in ("plain", "graph"):
                v = sorted(x["run_ms"] for x in rows if x["build"] == build and x["leg"] == leg)
                s[f"{k}_{leg}_run_ms"] = v[len(v) // 2]
                s[f"{k}_{leg}_spread"] = v[-1] / v[0]
        for leg in ("plain", "graph"):
            s[f"this_over_parent_{leg}"] = s[f"this_{leg}_run_ms"] / s[f"parent_{leg}_run_ms"]
        emit(s)


if __name__ == "__main__":
    main()
