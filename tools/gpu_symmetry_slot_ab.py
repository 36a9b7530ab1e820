"""A symmetry set per slot (P3HIP_FLAG_SYMMETRY_SLOT) against the plain engine fed host-rotated
features, interleaved A/B on one MI355X.

Engine part: wall time of p3hip_run alone (the slots are loaded, and their masks set, outside the timed call) for each
net at batch 1024 (default plan) and batch 8 (P3HIP_FLAG_LOW_LATENCY_ANY | P3HIP_FLAG_LAUNCH_GRAPH).  Legs, alternating
round by round in one process:
  plain        a plain engine, every slot's features rotated on the host by one random symmetry (the yardstick)
  slot_single  a SYMMETRY_SLOT engine with symmetry_rows = batch, identity features, one random symmetry per slot
  slot_root    the same with 1 slot in 32 at 0xFF, symmetry_rows = batch + 7 per such slot
With --parent-lib (and --out) the plain leg is also taken from that build of the library.  A process holds one build, so
the two builds alternate as processes: after a net's legs, `--rounds` times a one-round plain leg of this build
("build": "this commit, alternating") and then of the parent's ("build": "parent commit"), and a summary line
("alternating": true) with both medians and spreads per batch.  The chip's clock, power and limiter residency are sampled
beside every leg (p3achygo_amd/power_sampler.py, as the other A/B tools record it).

Host part (--selfplay): positions/s and host share of the self-play scheduler as tools/gpu_selfplay.py takes them, with
and without host_api.set_device_symmetry, legs alternating.

Prints one JSON line per leg and a summary per case: medians and spread (max - min) across rounds.

  python tools/gpu_symmetry_slot_ab.py --out profiles/symmetry_slot_ab.jsonl [--parent-lib libp3hip_parent.so]
  python tools/gpu_symmetry_slot_ab.py --selfplay --out profiles/symmetry_slot_ab.jsonl
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_symmetry_slot_ab.py --profile b12c256btl3 [--profile-leg plain]
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

NETS = ["b12c256btl3", "b14d96h3_transformer"]
SELFPLAY_NETS = ["b12c256btl3", "b12c128btl3"]
GRIDS = ("board", "stones_atari", "stones_two_liberties", "stones_three_liberties", "stones_laddered")


def rotate(recs, syms, fwd):
    """record r under symmetry syms[r], as host/features.h FillFeatures builds it"""
    out = recs.copy()
    for r, s in enumerate(syms):
        m = fwd[s].astype(np.int64)
        for g in GRIDS:
            out[g][r][m] = recs[g][r]
        li, lj = recs["last_moves"]["i"][r].astype(np.int64), recs["last_moves"]["j"][r].astype(np.int64)
        on = (li >= 0) & (li < 19) & (lj >= 0) & (lj < 19)
        t = m[np.where(on, li * 19 + lj, 0)]
        out["last_moves"]["i"][r] = np.where(on, t // 19, li)
        out["last_moves"]["j"][r] = np.where(on, t % 19, lj)
    return out


def weights(name, d):
    from p3achygo_amd import netspec
    cfg = netspec.get_config(name)
    path = os.path.join(d, name + ".p3w")
    netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
    return path


def cases():
    from p3achygo_amd import engine
    return [(1024, 0), (8, engine.FLAG_LOW_LATENCY_ANY | engine.FLAG_LAUNCH_GRAPH)]


def make_leg(kind, path, batch, flags, pos, syms, fwd):
    """(engine, load) — load() puts the batch into the slots, untimed"""
    from p3achygo_amd import engine
    if kind == "plain":
        eng = engine.HipEngine(path, batch, flags=flags)
        rot = rotate(pos, syms, fwd)
        return eng, lambda: eng.load_all(rot)
    masks = [1 << int(s) for s in syms]
    roots = 0
    if kind == "slot_root":
        for i in range(0, batch, 32):
            masks[i] = 0xFF
            roots += 1
    eng = engine.HipEngine(path, batch, flags=flags | engine.FLAG_SYMMETRY_SLOT, symmetry_rows=batch + 7 * roots)

    def load():
        eng.load_all(pos)
        for i, m in enumerate(masks):
            eng.set_slot_symmetries(i, m)
    return eng, load


def time_runs(eng, load, seconds):
    """ms per p3hip_run, the loads between the runs left out"""
    from p3achygo_amd.power_sampler import PowerSampler
    sampler = PowerSampler(0)   # (a leg without the chip's state beside it is no measurement: let it fail)
    sampler.start()
    total, n, t_end = 0.0, 0, time.perf_counter() + seconds
    while time.perf_counter() < t_end or n < 20:
        load()
        t0 = time.perf_counter()
        eng.RunInference()
        total += time.perf_counter() - t0
        n += 1
    chip = sampler.stop()
    return {"run_ms": total / n * 1e3, "runs": n, "graph_state": eng.graph_state(), "chip": chip}


def run_net(name, args, kinds, build):
    from p3achygo_amd import engine, features
    fwd = engine.symmetry_maps()[0]
    lines = []
    with tempfile.TemporaryDirectory() as d:
        path = weights(name, d)
        for batch, flags in cases():
            pos = features.random_positions(batch, seed=7, n_games=max(1, batch // 16))
            syms = np.random.default_rng(11).integers(0, 8, batch)
            legs = {k: make_leg(k, path, batch, flags, pos, syms, fwd) for k in kinds}
            for eng, load in legs.values():
                for _ in range(5):   # eager, capture, replays
                    load()
                    eng.RunInference()
            res = {k: [] for k in legs}
            for r in range(args.rounds):
                for kind, (eng, load) in legs.items():
                    x = time_runs(eng, load, args.leg_seconds)
                    x.update({"net": name, "batch": batch, "flags": flags, "round": r, "leg": kind, "build": build})
                    print(json.dumps(x), flush=True)
                    lines.append(x)
                    res[kind].append(x["run_ms"])
            for eng, _ in legs.values():
                eng.close()
            s = {"summary": True, "net": name, "batch": batch, "flags": flags, "build": build}
            for kind, v in res.items():
                v = sorted(v)
                s[kind + "_run_ms"] = v[len(v) // 2]
                s[kind + "_run_ms_spread"] = v[-1] - v[0]
            print(json.dumps(s), flush=True)
            lines.append(s)
    return lines


def run_selfplay(name, args):
    from p3achygo_amd import host_api
    lines = []
    with tempfile.TemporaryDirectory() as d:
        path = weights(name, d)
        host_api.set_groups(args.groups)
        res = {0: [], 1: []}
        try:
            for r in range(args.rounds):
                for dev in (0, 1):
                    host_api.set_device_symmetry(dev)
                    st = host_api.selfplay_run(path, 1024 * args.groups, args.threads, args.selfplay_seconds)
                    x = {"selfplay": True, "net": name, "round": r, "device_symmetry": dev, "groups": args.groups,
                         "threads": args.threads, "positions_per_s": st.positions / st.seconds,
                         "host_share": st.host_seconds / st.seconds, "run_ms": st.gpu_seconds / max(st.batches, 1) * 1e3,
                         "batches": st.batches}
                    print(json.dumps(x), flush=True)
                    lines.append(x)
                    res[dev].append(x)
        finally:
            host_api.set_device_symmetry(0)
        s = {"summary": True, "selfplay": True, "net": name}
        for dev, rows in res.items():
            for f in ("positions_per_s", "host_share"):
                v = sorted(x[f] for x in rows)
                s["%s_dev%d" % (f, dev)] = v[len(v) // 2]
                s["%s_dev%d_spread" % (f, dev)] = v[-1] - v[0]
        print(json.dumps(s), flush=True)
        lines.append(s)
    return lines


def profile(name, kind="slot_single", runs=30):
    """for a rocprofv3 --kernel-trace --stats run: runs of one leg at both cases, nothing else"""
    from p3achygo_amd import engine, features
    fwd = engine.symmetry_maps()[0]
    with tempfile.TemporaryDirectory() as d:
        path = weights(name, d)
        for batch, flags in cases():
            pos = features.random_positions(batch, seed=7, n_games=max(1, batch // 16))
            eng, load = make_leg(kind, path, batch, flags & ~engine.FLAG_LAUNCH_GRAPH, pos,
                                 np.random.default_rng(11).integers(0, 8, batch), fwd)
            for _ in range(runs):
                load()
                eng.RunInference()
            eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="*", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-seconds", type=float, default=0.5)
    ap.add_argument("--selfplay", action="store_true")
    ap.add_argument("--selfplay-seconds", type=float, default=6.0)
    ap.add_argument("--groups", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent-lib", default=None, help="libp3hip.so of the parent commit: its plain leg is recorded too")
    ap.add_argument("--step-timeout", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", metavar="NET")
    ap.add_argument("--profile-leg", default="slot_single", choices=("plain", "slot_single", "slot_root"))
    ap.add_argument("--one", metavar="NET", help=argparse.SUPPRESS)
    ap.add_argument("--build", default="this commit", help=argparse.SUPPRESS)
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.profile:
        return profile(args.profile, args.profile_leg)
    if args.one:
        if args.selfplay:
            lines = run_selfplay(args.one, args)
        else:
            kinds = ("plain",) if args.plain_only else ("plain", "slot_single", "slot_root")
            lines = run_net(args.one, args, kinds, args.build)
        if args.out:
            with open(args.out, "a") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")
        return
    nets = args.nets or (SELFPLAY_NETS if args.selfplay else NETS)
    if args.parent_lib and not args.out:
        sys.exit("--parent-lib needs --out: the alternating summary is taken from the file")
    for name in nets:
        steps = [("this commit", None, args.rounds)]
        if args.parent_lib and not args.selfplay:
            for _ in range(args.rounds):
                steps += [("this commit, alternating", None, 1), ("parent commit", os.path.abspath(args.parent_lib), 1)]
        for build, lib, rounds in steps:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--rounds", str(rounds), "--leg-seconds",
                   str(args.leg_seconds), "--build", build, "--selfplay-seconds", str(args.selfplay_seconds),
                   "--groups", str(args.groups), "--threads", str(args.threads)]
            if build != "this commit":
                cmd.append("--plain-only")
            if args.selfplay:
                cmd.append("--selfplay")
            if args.out:
                cmd += ["--out", args.out]
            env = dict(os.environ)
            if lib:
                env["P3HIP_LIB"] = lib
            r = subprocess.run(cmd, env=env, timeout=args.step_timeout or None)
            if r.returncode != 0:
                sys.exit(f"step {name} ({build}) failed with exit status {r.returncode}: stopping")
        if args.parent_lib and not args.selfplay:
            rows = [json.loads(ln) for ln in open(args.out)]
            for batch in sorted({x["batch"] for x in rows if x.get("net") == name and "leg" in x}):
                s = {"summary": True, "alternating": True, "net": name, "batch": batch}
                for build, key in (("this commit, alternating", "this"), ("parent commit", "parent")):
                    v = sorted(x["run_ms"] for x in rows if x.get("net") == name and x.get("batch") == batch and
                               x.get("build") == build and x.get("leg") == "plain")
                    s[key + "_plain_run_ms"] = v[len(v) // 2]
                    s[key + "_plain_run_ms_spread"] = v[-1] - v[0]
                print(json.dumps(s), flush=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(s) + "\n")


if __name__ == "__main__":
    main()
