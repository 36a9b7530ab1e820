"""Cost of symmetry-averaged evaluation (P3HIP_FLAG_SYMMETRY_AVG).

For each trunk and slot count S: the wall time of p3hip_run on a k = 8 engine of S slots (H2D of S records, expand,
forward pass over 8 S rows, reduce, D2H of S records) against p3hip_run on a plain engine of 8 S slots loaded with
the same 8 S positions (H2D and D2H of 8 S records).  Prints one JSON line per case and writes them to --out.

    python tools/gpu_symmetry_avg_bench.py [--iters N] [--nets a,b] [--slots 128,1024] [--out profiles/x.jsonl]

The share of k_sym_expand and k_sym_reduce comes from a run of its own under rocprofv3 (the program after `--`):
    rocprofv3 --kernel-trace --stats -d DIR -o symavg -- python tools/gpu_symmetry_avg_bench.py --iters 3
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from p3achygo_amd import engine, features, netspec  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--nets", default="b12c256btl3,b14c384btl3,b14d96h3_transformer")
ap.add_argument("--slots", default="128,1024")
ap.add_argument("--out", default="")
args = ap.parse_args()


def weights(name, d):
    path = os.path.join(d, name + ".p3w")
    if name in netspec.CONFIGS:
        cfg = netspec.CONFIGS[name]
    else:
        cfg = netspec.TRANSFORMER_CONFIGS[name]
    netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
    return path


def time_runs(eng, iters):
    eng.RunInference()   # warm-up; the slots stay loaded-and-unfetched, so every run evaluates all of them again
    eng.RunInference()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        eng.RunInference()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3


lines = []
d = tempfile.mkdtemp()
for name in args.nets.split(","):
    path = weights(name, d)
    for slots in (int(s) for s in args.slots.split(",")):
        pos = features.random_positions(slots, seed=7)
        sym = engine.HipEngine(path, slots, flags=engine.FLAG_SYMMETRY_AVG)
        sym.load_all(pos)
        sym_med, sym_min = time_runs(sym, args.iters)
        sym.close()
        fwd = engine.symmetry_maps()[0]
        import symavg_restatement as sr
        copies = sr.expand(pos, 0xFF, fwd)
        plain = engine.HipEngine(path, 8 * slots)
        plain.load_all(copies)
        plain_med, plain_min = time_runs(plain, args.iters)
        plain.close()
        rec = {"net": name, "slots": slots, "rows": 8 * slots, "iters": args.iters,
               "sym_run_ms_median": round(sym_med, 3), "sym_run_ms_min": round(sym_min, 3),
               "plain_8x_run_ms_median": round(plain_med, 3), "plain_8x_run_ms_min": round(plain_min, 3),
               "ratio_median": round(sym_med / plain_med, 4)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
if args.out:
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
