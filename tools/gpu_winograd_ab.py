"""fp16, INT8 for the 3x3 convs only (P3HIP_FLAG_INT8_CONV3) and the Winograd plan (P3HIP_FLAG_WINOGRAD), interleaved A/B
on one MI355X, on tools/gpu_int8_conv3_ab.py's frame.

For each trunk and batch size the three engines are built from the same seeded .p3w; the INT8 engine is calibrated on
tests/int8_restatement.calibration_batches().  Legs alternate fp16, int8_conv3, winograd, fp16, ... for --rounds rounds
(at least three); each leg times `--steps` device-resident forward passes (engine only: no H2D / D2H) with the chip's
clock, power and limiter residency sampled beside it (p3achygo_amd/power_sampler.py), then the 3x3 launch alone
(p3hip_time_trunk_kernel: k_lconv / k_lconv_any, k_lconv_i8 / k_lconv_i8_any, k_wconv; the average over the 3x3 launches
of a pass).  Prints one JSON line per leg and a summary per (trunk, batch): medians, the spread (max / min) of every leg's
forward time, `winograd_over_fp16_forward_time`, and per leg the 3x3 launch's achieved fraction of the fp16 MFMA peak
(2.5 PFLOP/s dense, the datasheet's), counted in the FLOPs of the direct conv.  There is no threshold.

With --parent-lib (and --out) the fp16 leg is also taken from that build of the library, to show that the fp16 plan did not
move: the builds alternate as processes, as in tools/gpu_int8_conv3_ab.py.  Every (trunk, batch) is a step of its own: it
runs in a child process of this tool, under --step-timeout seconds when given, and the tool stops at the first step that
fails or runs out of time.

  python tools/gpu_winograd_ab.py --out profiles/winograd_ab.jsonl [--parent-lib libp3hip_parent.so]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_int8_ab import leg  # noqa: E402
from gpu_int8_any_ab import calibrate, chip_of, median  # noqa: E402
from gpu_int8_conv3_ab import n3x3  # noqa: E402

NETS = ["b14c384btl3", "b10c384nbt", "b15c192_classic", "b14c320btl3", "b10c512nbt"]
LEGS = ("fp16", "int8_conv3", "winograd")
FP16_PEAK = 2.5e15   # dense fp16 MFMA, FLOP/s (datasheet)


def _flags(engine):
    return {"fp16": 0, "int8_conv3": engine.FLAG_INT8_CONV3, "winograd": engine.FLAG_WINOGRAD}


def run_fp16(path, cfg, batch, args):
    """one fp16 leg of whatever build P3HIP_LIB names (the alternating processes of --parent-lib)"""
    from p3achygo_amd import engine, features
    pos = features.random_positions(batch, seed=7, n_games=max(1, batch // 16))
    eng = engine.HipEngine(path, batch)
    eng.load_all(pos)
    eng.upload()
    x = leg(eng, batch, args.steps, args.kernel_iters, "kernel")
    eng.close()
    x.update({"net": cfg.name, "batch": batch, "precision": "fp16", "build": args.build, "flag": "winograd"})
    print(json.dumps(x), flush=True)
    return [x]


def run_step(path, cfg, batch, args):
    from p3achygo_amd import engine, features
    pos = features.random_positions(batch, seed=7, n_games=max(1, batch // 16))
    flags = _flags(engine)
    engines = {k: engine.HipEngine(path, batch, flags=flags[k]) for k in LEGS}
    plans = {k: engine.debug_plan(path, flags[k])[0] for k in LEGS}
    for k, eng in engines.items():
        if k == "int8_conv3":
            calibrate(eng)
        eng.load_all(pos)
        eng.upload()
    lines, res = [], {k: [] for k in LEGS}
    for r in range(args.rounds):
        for kind in LEGS:
            x = leg(engines[kind], batch, args.steps, args.kernel_iters, "kernel")
            x.update({"net": cfg.name, "batch": batch, "round": r, "precision": kind, "plan": plans[kind], "flag": "winograd"})
            print(json.dumps(x), flush=True)
            lines.append(x)
            res[kind].append(x)
    for eng in engines.values():
        eng.close()
    s = {"summary": True, "net": cfg.name, "batch": batch, "flag": "winograd", "rounds": args.rounds, "k3x3_launches": n3x3(cfg)}
    for kind in LEGS:
        s[kind + "_plan"] = plans[kind]
        s[kind + "_pos_per_s"] = median(res[kind], "pos_per_s")
        s[kind + "_ms_per_forward"] = median(res[kind], "ms_per_forward")
        s[kind + "_forward_spread"] = (max(v["ms_per_forward"] for v in res[kind]) / min(v["ms_per_forward"] for v in res[kind]))
        s[kind + "_k3x3"] = res[kind][0]["kernel_name"]
        s[kind + "_k3x3_ms"] = median(res[kind], "kernel_ms")
        s[kind + "_k3x3_direct_flops"] = res[kind][0]["kernel_flops"]
        s[kind + "_k3x3_fraction_of_fp16_peak"] = res[kind][0]["kernel_flops"] / (s[kind + "_k3x3_ms"] * 1e-3) / FP16_PEAK
        s[kind + "_rest_ms"] = s[kind + "_ms_per_forward"] - s["k3x3_launches"] * s[kind + "_k3x3_ms"]
        s[kind + "_chip"] = chip_of(res[kind])
    s["winograd_over_fp16_forward_time"] = s["winograd_ms_per_forward"] / s["fp16_ms_per_forward"]
    s["conv3_over_fp16_forward_time"] = s["int8_conv3_ms_per_forward"] / s["fp16_ms_per_forward"]
    s["winograd_over_fp16_k3x3_time"] = s["winograd_k3x3_ms"] / s["fp16_k3x3_ms"]
    print(json.dumps(s), flush=True)
    lines.append(s)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="*", default=NETS)
    ap.add_argument("--batches", nargs="+", type=int, default=[1024, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--kernel-iters", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=0, help="seconds: the time limit of each (trunk, batch) step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add the lines to --out instead of replacing it")
    ap.add_argument("--parent-lib", default=None, help="libp3hip.so of the parent commit: its fp16 leg is recorded too")
    ap.add_argument("--one", nargs=2, metavar=("NET", "BATCH"), help=argparse.SUPPRESS)
    ap.add_argument("--build", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.rounds < 3:
        sys.exit("--rounds: at least three")
    from p3achygo_amd import netspec
    if args.one:
        name, batch = args.one[0], int(args.one[1])
        with tempfile.TemporaryDirectory() as d:
            cfg = netspec.get_config(name)
            path = os.path.join(d, name + ".p3w")
            netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
            lines = run_fp16(path, cfg, batch, args) if args.build else run_step(path, cfg, batch, args)
        if args.out:
            with open(args.out, "a") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")
        return
    if args.out and os.path.exists(args.out) and not args.append:
        os.remove(args.out)
    if args.parent_lib and not args.out:
        sys.exit("--parent-lib needs --out: the alternating summary is taken from the file")
    for name in args.nets:
        for batch in args.batches:
            steps = [(None, None)]
            if args.parent_lib:
                steps += [("this commit, alternating", None), ("parent commit", os.path.abspath(args.parent_lib))] * args.rounds
            for build, lib in steps:
                cmd = [sys.executable, os.path.abspath(__file__), "--one", name, str(batch), "--rounds", str(args.rounds),
                       "--steps", str(args.steps), "--kernel-iters", str(args.kernel_iters)]
                if build:
                    cmd += ["--build", build]
                if args.out:
                    cmd += ["--out", args.out]
                env = dict(os.environ)
                if lib:
                    env["P3HIP_LIB"] = lib
                t0 = time.time()
                r = subprocess.run(cmd, env=env, timeout=args.step_timeout or None)
                if r.returncode != 0:
                    sys.exit(f"step {name} batch {batch} ({build}) failed with exit status {r.returncode}: stopping")
                print(f"# {name} batch {batch}{' (' + build + ')' if build else ''}: {time.time() - t0:.0f} s", flush=True)
            if args.parent_lib:
                rows = [json.loads(ln) for ln in open(args.out)]
                s = {"summary": True, "alternating": True, "net": name, "batch": batch, "flag": "winograd"}
                for build, key in (("this commit, alternating", "this"), ("parent commit", "parent")):
                    v = sorted(x["ms_per_forward"] for x in rows if x.get("net") == name and x.get("batch") == batch and
                               x.get("build") == build)
                    s[key + "_fp16_ms_per_forward"], s[key + "_fp16_spread_ms"] = v[len(v) // 2], v[-1] - v[0]
                print(json.dumps(s), flush=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(s) + "\n")


if __name__ == "__main__":
    main()
