"""The default transformer plan against the low-latency plan of the transformer trunks (P3HIP_FLAG_LOW_LATENCY_TFM) at small
batches, interleaved A/B on one MI355X.  The default leg runs the kernels of csrc/transformer.hip, which the flag leaves as
they are; the flagged leg returns the same bits (tests/test_low_latency_tfm_gpu.py), so this tool measures time alone.

For each trunk and batch size two engines are built from the same seeded .p3w, both with P3HIP_FLAG_LAUNCH_GRAPH and a
static batch of exactly that size (the shape of a GTP service or an evaluation match: batch_size = search threads).  A
trunk is a name of netspec or b<blocks>d<width>h<heads> (b14d192h6: random-init weights of that shape).  Legs
alternate default, low_latency, default, ...  A leg measures two things, each over enough passes to last --leg-seconds:
  forward_ms   one device-resident forward pass (p3hip_forward_resident + sync per pass: what a searcher waits for)
  run_ms       one end-to-end run: the slots loaded, p3hip_run (H2D, pass, D2H)
(the captured graph serves the pass it was captured for, so each plan has one engine for either measurement, warmed
with that measurement's own calls until the graph replays) with the chip's clock, power and limiter residency sampled
beside the forward window (p3achygo_amd/power_sampler.py, as the other A/B tools record it).  Prints one JSON line per
leg, a summary per (trunk, batch) with the split the chooser takes on --cus CUs (p3hip_debug_tfm_split), the medians, the
spread across rounds (max - min) and the ratios low_latency / default, and per trunk the crossover: the smallest batch
at which the default plan's median forward pass is the faster one.  `forward_win`: the low-latency median is below the
default one by more than the larger of the two legs' spreads.  Where the split is (1, 64) both legs launch the same
kernels.

Every trunk is a step of its own: it runs in a child process of this tool, under --step-timeout seconds when given, and
the tool stops at the first step that fails or runs out of time.

  python tools/gpu_low_latency_tfm_ab.py --out profiles/low_latency_tfm_ab.jsonl
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

NETS = ["b14d96h3_transformer"]
BATCHES = [1, 2, 4, 8, 16, 32, 64, 256]


def config(name):
    from p3achygo_amd import netspec
    m = re.fullmatch(r"b(\d+)d(\d+)h(\d+)", name)
    return netspec.transformer_config(name, int(m.group(1)), int(m.group(2)), int(m.group(3))) if m else netspec.get_config(name)


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
    from p3achygo_amd.power_sampler import PowerSampler
    feng, reng = engs

    def forward():
        feng.forward_resident(batch)
        feng.sync()

    def run():
        reng.load_all(pos)
        reng.RunInference()
    try:
        sampler = PowerSampler(0)
        sampler.start()
    except Exception:   # noqa: BLE001
        sampler = None
    fwd, nf = timed(forward, seconds)
    power = sampler.stop() if sampler is not None else None
    e2e, nr = timed(run, seconds)
    return {"forward_ms": fwd, "forward_passes": nf, "run_ms": e2e, "runs": nr,
            "graph_state": [feng.graph_state(), reng.graph_state()], "chip": power}


def run_net(name, args):
    from p3achygo_amd import engine, features, netspec
    lines = []
    with tempfile.TemporaryDirectory() as d:
        cfg = config(name)
        path = os.path.join(d, name + ".p3w")
        netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
        med = {}
        for batch in args.batches:
            pos = features.random_positions(batch, seed=7, n_games=max(1, batch // 16))
            flags = {"default": engine.FLAG_LAUNCH_GRAPH, "low_latency": engine.FLAG_LAUNCH_GRAPH | engine.FLAG_LOW_LATENCY_TFM}
            engs = {k: (engine.HipEngine(path, batch, flags=f), engine.HipEngine(path, batch, flags=f)) for k, f in flags.items()}
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
                    x.update({"net": name, "batch": batch, "round": r, "plan": kind})
                    print(json.dumps(x), flush=True)
                    lines.append(x)
                    res[kind].append(x)
            for pair in engs.values():
                for eng in pair:
                    eng.close()
            s = {"summary": True, "net": name, "batch": batch,
                 "split": list(engine.debug_tfm_split(batch, cfg.bottleneck_channels, args.cus))}
            for kind, rows in res.items():
                for f in ("forward_ms", "run_ms"):
                    v = sorted(x[f] for x in rows)
                    s["%s_%s" % (kind, f)] = v[len(v) // 2]
                    s["%s_%s_spread" % (kind, f)] = v[-1] - v[0]
                chips = [x["chip"] for x in rows if x.get("chip")]
                s[kind + "_chip"] = chips[len(chips) // 2] if chips else None
            for f in ("forward_ms", "run_ms"):
                s["ratio_" + f] = s["low_latency_" + f] / s["default_" + f]
            s["forward_win"] = (s["default_forward_ms"] - s["low_latency_forward_ms"] >
                                max(s["default_forward_ms_spread"], s["low_latency_forward_ms_spread"]))
            s["run_win"] = s["low_latency_run_ms"] < s["default_run_ms"]
            print(json.dumps(s), flush=True)
            lines.append(s)
            med[batch] = s["ratio_forward_ms"]
        slower = [b for b in sorted(med) if med[b] >= 1.0]
        c = {"crossover": True, "net": name, "batches": sorted(med),
             "first_batch_default_is_faster": slower[0] if slower else None}
        print(json.dumps(c), flush=True)
        lines.append(c)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="*", default=NETS)
    ap.add_argument("--batches", nargs="+", type=int, default=BATCHES)
    ap.add_argument("--cus", type=int, default=256, help="CUs of the device: the split reported is the chooser's for them")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg-seconds", type=float, default=0.3)
    ap.add_argument("--step-timeout", type=int, default=0, help="seconds: the time limit of each trunk's step")
    ap.add_argument("--out", default=None)
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
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--rounds", str(args.rounds), "--cus", str(args.cus), "--leg-seconds",
               str(args.leg_seconds), "--batches"] + [str(b) for b in args.batches]
        if args.out:
            cmd += ["--out", args.out]
        t0 = time.time()
        r = subprocess.run(cmd, timeout=args.step_timeout or None)
        if r.returncode != 0:
            sys.exit(f"step {name} failed with exit status {r.returncode}: stopping")
        print(f"# {name}: {time.time() - t0:.0f} s", flush=True)


if __name__ == "__main__":
    main()
