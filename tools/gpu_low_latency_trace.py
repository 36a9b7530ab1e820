"""What a low-latency forward pass spends where: run under `rocprofv3 --kernel-trace --stats` (a run of its own, never
beside a timing), it does `--passes` device-resident forward passes of one trunk at one batch size on a
P3HIP_FLAG_LOW_LATENCY engine (launch graph on, as tools/gpu_low_latency_ab.py times it) and prints the wall time per
pass, so that the trace's kernel times can be set against it: the share of k_sconv, of the stem, dense and heads
kernels (unsplit: one position per workgroup), and of the gaps between launches.

  rocprofv3 --kernel-trace --stats -d OUTPUT_DIR -o ll -- python tools/gpu_low_latency_trace.py
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="b12c256btl3")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--default-plan", action="store_true", help="the default plan instead (for comparison)")
    args = ap.parse_args()
    from p3achygo_amd import engine, features, netspec
    with tempfile.TemporaryDirectory() as d:
        cfg = netspec.get_config(args.net)
        path = os.path.join(d, args.net + ".p3w")
        netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
        flags = engine.FLAG_LAUNCH_GRAPH | (0 if args.default_plan else engine.FLAG_LOW_LATENCY)
        eng = engine.HipEngine(path, args.batch, flags=flags)
        eng.load_all(features.random_positions(args.batch, seed=7))
        eng.upload()
        for _ in range(4):
            eng.forward_resident(args.batch)
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(args.passes):
            eng.forward_resident(args.batch)
            eng.sync()
        dt = time.perf_counter() - t0
        print(json.dumps({"net": args.net, "batch": args.batch, "plan": "default" if args.default_plan else "low_latency",
                          "passes": args.passes + 4, "ms_per_pass_under_the_profiler": dt / args.passes * 1e3,
                          "graph_state": eng.graph_state()}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
