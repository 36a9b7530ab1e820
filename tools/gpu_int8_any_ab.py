"""fp16 against calibrated INT8 at any width (P3HIP_FLAG_INT8_ANY), interleaved A/B on one MI355X, and the runtime-width
INT8 kernels against the templated ones on the one net both run.

For each trunk and batch size the two engines are built from the same seeded .p3w; the INT8 engine is calibrated on
tests/int8_restatement.calibration_batches().  Legs alternate fp16, int8, fp16, int8, ...; each leg times `--steps`
device-resident forward passes (engine only: no H2D / D2H) with the chip's clock, power and limiter residency sampled
beside it (p3achygo_amd/power_sampler.py, as bench.py does), then the trunk kernel alone (p3hip_time_trunk_kernel: on the
INT8 leg the 3x3 k_lconv_i8_any, on the fp16 leg the 3x3 k_lconv_any or, where the fp16 plan is the fused block kernel,
the block launch; each leg's own FLOPs per launch).  Prints one JSON line per leg and a summary per (trunk, batch).

--forms NET (default b14c384btl3, "" to skip): P3HIP_FLAG_INT8_ANY with P3HIP_CONV_ANY=1 (k_lconv_i8_any) against
P3HIP_FLAG_INT8 (the templated k_lconv_i8) on that net, interleaved the same way; the summary's
`any_over_templated_forward_time` is the runtime-width kernels' forward time as a ratio of the templated ones'.  There is
no threshold for it.  (P3HIP_CONV_ANY is read when an engine is created: both engines live in this one process.)

Every (trunk, batch) is a step of its own: it runs in a child process of this tool, under --step-timeout seconds when
given, and the tool stops at the first step that fails or runs out of time.

  python tools/gpu_int8_any_ab.py --out profiles/int8_any_ab.jsonl
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

from gpu_int8_ab import PEAK_F16, PEAK_I8, leg  # noqa: E402

NETS = ["b8c128nbt", "b12c256nbt", "b12c192btl3", "b14c320btl3", "b10c512nbt"]


def calibrate(eng):
    import int8_restatement as ir
    for cal in ir.calibration_batches():
        eng.load_all(cal)
        eng.int8_calibrate()
        for i in range(len(cal)):
            eng.GetBatch(i)


def median(rows, field):
    return sorted(v[field] for v in rows)[len(rows) // 2]


def chip_of(rows):
    chips = [v["chip"] for v in rows if v.get("chip")]
    return chips[len(chips) // 2] if chips else None


def run_pair(path, name, batch, args, forms):
    """the legs and the summary of one (trunk, batch).  forms: INT8 templated against INT8_ANY + P3HIP_CONV_ANY=1"""
    from p3achygo_amd import engine, features
    pos = features.random_positions(batch, seed=7, n_games=max(1, batch // 16))
    os.environ.pop("P3HIP_CONV_ANY", None)
    a_name, b_name = ("int8_templated", "int8_any") if forms else ("fp16", "int8_any")
    a = engine.HipEngine(path, batch, flags=engine.FLAG_INT8 if forms else 0)
    if forms:
        os.environ["P3HIP_CONV_ANY"] = "1"
    b = engine.HipEngine(path, batch, flags=engine.FLAG_INT8_ANY)
    os.environ.pop("P3HIP_CONV_ANY", None)
    for eng in ((a, b) if forms else (b,)):
        calibrate(eng)
    for eng in (a, b):
        eng.load_all(pos)
        eng.upload()
    lines, res = [], {a_name: [], b_name: []}
    for r in range(args.rounds):
        for kind, eng in ((a_name, a), (b_name, b)):
            x = leg(eng, batch, args.steps, args.kernel_iters, "kernel")
            x.update({"net": name, "batch": batch, "round": r, "precision": kind, "flag": "int8_any", "forms": forms})
            print(json.dumps(x), flush=True)
            lines.append(x)
            res[kind].append(x)
    a.close()
    b.close()
    s = {"summary": True, "net": name, "batch": batch, "flag": "int8_any", "forms": forms}
    for kind in (a_name, b_name):
        s[kind + "_pos_per_s"] = median(res[kind], "pos_per_s")
        s[kind + "_ms_per_forward"] = median(res[kind], "ms_per_forward")
        s[kind + "_forward_spread"] = (max(v["ms_per_forward"] for v in res[kind]) /
                                       min(v["ms_per_forward"] for v in res[kind]))
        s[kind + "_kernel"] = res[kind][0]["kernel_name"]
        s[kind + "_kernel_ms"] = median(res[kind], "kernel_ms")
        peak = PEAK_F16 if kind == "fp16" else PEAK_I8
        s[kind + "_kernel_of_peak"] = res[kind][0]["kernel_flops"] / (s[kind + "_kernel_ms"] * 1e-3) / peak
        s[kind + "_chip"] = chip_of(res[kind])
    if forms:
        s["any_over_templated_forward_time"] = s["int8_any_ms_per_forward"] / s["int8_templated_ms_per_forward"]
        s["any_over_templated_k3x3_time"] = s["int8_any_kernel_ms"] / s["int8_templated_kernel_ms"]
    else:
        s["speedup_forward"] = s["int8_any_pos_per_s"] / s["fp16_pos_per_s"]
    print(json.dumps(s), flush=True)
    lines.append(s)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="*", default=NETS)
    ap.add_argument("--forms", default="b14c384btl3")
    ap.add_argument("--batches", nargs="+", type=int, default=[1024, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--kernel-iters", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=0, help="seconds: the time limit of each (trunk, batch) step")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", nargs=3, metavar=("NET", "BATCH", "FORMS"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    from p3achygo_amd import netspec
    if args.one:
        name, batch, forms = args.one[0], int(args.one[1]), args.one[2] == "1"
        with tempfile.TemporaryDirectory() as d:
            cfg = netspec.get_config(name)
            path = os.path.join(d, name + ".p3w")
            netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
            lines = run_pair(path, name, batch, args, forms)
        if args.out:
            with open(args.out, "a") as f:
                for x in lines:
                    f.write(json.dumps(x) + "\n")
        return
    if args.out and os.path.exists(args.out):
        os.remove(args.out)
    steps = [(n, b, False) for n in args.nets for b in args.batches] + \
            ([(args.forms, b, True) for b in args.batches] if args.forms else [])
    for name, batch, forms in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, str(batch), "1" if forms else "0",
               "--rounds", str(args.rounds), "--steps", str(args.steps), "--kernel-iters", str(args.kernel_iters)]
        if args.out:
            cmd += ["--out", args.out]
        t0 = time.time()
        r = subprocess.run(cmd, timeout=args.step_timeout or None)
        if r.returncode != 0:
            sys.exit(f"step {name} batch {batch} failed with exit status {r.returncode}: stopping")
        print(f"# {name} batch {batch}{' (forms)' if forms else ''}: {time.time() - t0:.0f} s", flush=True)


if __name__ == "__main__":
    main()
