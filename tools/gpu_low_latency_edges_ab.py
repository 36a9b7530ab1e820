"""The split stem, broadcast dense and heads of the low-latency plans (csrc/edge_split.hip) against
the unsplit launches, interleaved A/B on one MI355X.

For each trunk and batch size the two legs are engines with the same low-latency flag (P3HIP_FLAG_LOW_LATENCY for a conv
trunk, P3HIP_FLAG_LOW_LATENCY_TFM for a transformer) and P3HIP_FLAG_LAUNCH_GRAPH, from the same seeded .p3w, with a static
batch of exactly that size: `split` takes the chooser's parts (p3hip_debug_edge_split), `unsplit` was created under
P3HIP_EDGE_SPLIT=0, the launches of the engine before the split forms existed (--force s,d,h: the split leg takes these
parts at every batch instead, to price one level of a piece).  A trunk is a name of netspec or
b<blocks>d<width>h<heads>[v<V>] (b14d384h6v80: random-init transformer weights of that shape).  Legs alternate split,
unsplit, split, ...  A leg measures two things, each over enough passes to last --leg-seconds:
  forward_ms   one device-resident forward pass (p3hip_forward_resident + sync per pass)
  run_ms       one end-to-end run: the slots loaded, p3hip_run (H2D, pass, D2H)
Prints one JSON line per leg and a summary per (trunk, batch): the medians, the spread across rounds (max - min), the
chooser's parts, the ratios split / unsplit, `forward_win` (the split median is below the unsplit one by more than the
larger of the two spreads) and `forward_loss` (above it by more than that).

Every trunk is a step of its own: it runs in a child process of this tool, one GPU process at a time, under
--step-timeout seconds when given, and the tool stops at the first step that fails or runs out of time.

  python tools/gpu_low_latency_edges_ab.py --out profiles/low_latency_edges_ab.jsonl
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NETS = ["b12c256btl3", "b14c384btl3", "b15c192_classic", "b12c128btl3", "b14d96h3_transformer", "b14d384h6v80"]
BATCHES = [1, 2, 4, 8, 16, 32]
LEGS = ("split", "unsplit")


def config(name):
    from p3achygo_amd import netspec
    m = re.fullmatch(r"b(\d+)d(\d+)h(\d+)(?:v(\d+))?", name)
    if not m:
        return netspec.get_config(name)
    return netspec.transformer_config(name, int(m.group(1)), int(m.group(2)), int(m.group(3)), c_val=int(m.group(4) or 64))


def timed(fn, seconds, floor=20):
    """ms per call of fn over a window of at least `seconds` (the count comes from a short trial)"""
    t0 = time.perf_counter()
    for _ in range(floor):
        fn()
    trial = (time.perf_counter() - t0) / floor
    n = max(floor, int(seconds / trial * 1.1) + 1)
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n * 1e3, n


def leg(engs, pos, batch, seconds):
    feng, reng = engs

    def forward():
        feng.forward_resident(batch)
        feng.sync()

    def run():
        reng.load_all(pos)
        reng.RunInference()
    fwd, nf = timed(forward, seconds)
    e2e, nr = timed(run, seconds)
    return {"forward_ms": fwd, "forward_passes": nf, "run_ms": e2e, "runs": nr,
            "graph_state": [feng.graph_state(), reng.graph_state()]}


def make_engines(path, batch, flags, kind, force=None):
    """P3HIP_EDGE_SPLIT is read at p3hip_create"""
    from p3achygo_amd import engine
    old = os.environ.pop("P3HIP_EDGE_SPLIT", None)
    try:
        if kind == "unsplit":
            os.environ["P3HIP_EDGE_SPLIT"] = "0"
        elif force:
            os.environ["P3HIP_EDGE_SPLIT"] = force
        return engine.HipEngine(path, batch, flags=flags), engine.HipEngine(path, batch, flags=flags)
    finally:
        os.environ.pop("P3HIP_EDGE_SPLIT", None)
        if old is not None:
            os.environ["P3HIP_EDGE_SPLIT"] = old


def run_net(name, args):
    from p3achygo_amd import engine, features, netspec
    lines = []
    with tempfile.TemporaryDirectory() as d:
        cfg = config(name)
        path = os.path.join(d, name + ".p3w")
        netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
        tfm = cfg.block_type == "transformer"
        flags = engine.FLAG_LAUNCH_GRAPH | (engine.FLAG_LOW_LATENCY_TFM if tfm else engine.FLAG_LOW_LATENCY)
        c_pad = (128 if cfg.channels <= 128 else 256 if cfg.channels <= 256 else 384) if tfm else (cfg.channels + 63) // 64 * 64
        for batch in args.batches:
            pos = features.random_positions(batch, seed=7, n_games=max(1, batch // 16))
            engs = {k: make_engines(path, batch, flags, k, args.force) for k in LEGS}
            for feng, reng in engs.values():
                feng.load_all(pos)
                feng.upload()
                for _ in range(4):        # eager, capture, replay, replay
                    feng.forward_resident(batch)
                    reng.load_all(pos)
                    reng.RunInference()
                feng.sync()
            res = {k: [] for k in engs}
            for r in range(args.rounds):
                for kind, eng in engs.items():
                    x = leg(eng, pos, batch, args.leg_seconds)
                    x.update({"net": name, "batch": batch, "round": r, "leg": kind})
                    print(json.dumps(x), flush=True)
                    lines.append(x)
                    res[kind].append(x)
            for pair in engs.values():
                for eng in pair:
                    eng.close()
            s = {"summary": True, "net": name, "batch": batch,
                 "parts": [int(v) for v in args.force.split(",")] if args.force else list(engine.debug_edge_split(batch, c_pad))}
            for kind, rows in res.items():
                for f in ("forward_ms", "run_ms"):
                    v = sorted(x[f] for x in rows)
                    s["%s_%s" % (kind, f)] = v[len(v) // 2]
                    s["%s_%s_spread" % (kind, f)] = v[-1] - v[0]
            for f in ("forward_ms", "run_ms"):
                s["ratio_" + f] = s["split_" + f] / s["unsplit_" + f]
            spread = max(s["split_forward_ms_spread"], s["unsplit_forward_ms_spread"])
            s["forward_win"] = s["unsplit_forward_ms"] - s["split_forward_ms"] > spread
            s["forward_loss"] = s["split_forward_ms"] - s["unsplit_forward_ms"] > spread
            print(json.dumps(s), flush=True)
            lines.append(s)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="*", default=NETS)
    ap.add_argument("--batches", nargs="+", type=int, default=BATCHES)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-seconds", type=float, default=0.3)
    ap.add_argument("--step-timeout", type=int, default=0, help="seconds: the time limit of each trunk's step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--force", metavar="s,d,h", help="the split leg's P3HIP_EDGE_SPLIT instead of the chooser's parts")
    ap.add_argument("--one", metavar="NET", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        lines = run_net(args.one, args)
        if args.out:
            with open(args.out, "a") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")
        return
    if args.out and os.path.exists(args.out):
        os.remove(args.out)
    for name in args.nets:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--rounds", str(args.rounds), "--leg-seconds",
               str(args.leg_seconds), "--batches"] + [str(b) for b in args.batches]
        if args.out:
            cmd += ["--out", args.out]
        if args.force:
            cmd += ["--force", args.force]
        t0 = time.time()
        r = subprocess.run(cmd, timeout=args.step_timeout or None)
        if r.returncode != 0:
            sys.exit(f"step {name} failed with exit status {r.returncode}: stopping")
        print(f"# {name}: {time.time() - t0:.0f} s", flush=True)


if __name__ == "__main__":
    main()
