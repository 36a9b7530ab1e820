"""What P3HIP_FLAG_AUX costs: the same binary with and without the flag, interleaved A/B on one MI355X.

For each trunk and batch size the two engines are built from the same seeded .p3w.  Legs alternate plain, aux, plain,
aux, ...; each leg times `--steps` device-resident forward passes (engine only: no H2D / D2H) with the chip's clock,
power and limiter residency sampled beside it (p3achygo_amd/power_sampler.py, as bench.py does), then the trunk kernel
alone (p3hip_time_trunk_kernel), which the flag does not touch.  The aux leg adds, per forward pass, k_heads_aux and, on
trunks whose heads kernel has the head convs inside (k_headsx), the head-conv launch that feeds it.
Prints one JSON line per leg and a summary per (trunk, batch) with the medians, the ratio aux / plain of the time per
forward pass, and each leg's run-to-run spread (max - min over its rounds, relative to the median); --out writes them all.
The plain leg is the yardstick: run with --legs plain from a checkout of another commit (this file copied into its tools/), it
times that build the same way, aux-less engine.py included.

  python tools/gpu_aux_ab.py --out profiles/aux_ab.jsonl
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="+", default=["b12c256btl3", "b14c384btl3"])
    ap.add_argument("--batches", nargs="+", type=int, default=[1024])
    ap.add_argument("--legs", nargs="+", choices=["plain", "aux"], default=["plain", "aux"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kernel-iters", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gpu_int8_ab import leg
    from p3achygo_amd import engine, features, netspec
    lines = []
    with tempfile.TemporaryDirectory() as d:
        for name in args.nets:
            cfg = netspec.get_config(name)
            path = os.path.join(d, name + ".p3w")
            netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
            for batch in args.batches:
                pos = features.random_positions(batch, seed=7, n_games=max(1, batch // 16))
                # (run from a checkout without the flag, engine has no FLAG_AUX: the plain leg needs none)
                engs = {k: engine.HipEngine(path, batch, flags=0 if k == "plain" else engine.FLAG_AUX) for k in args.legs}
                for eng in engs.values():
                    eng.load_all(pos)
                    eng.upload()
                res = {k: [] for k in engs}
                for r in range(args.rounds):
                    for kind, eng in engs.items():
                        x = leg(eng, batch, args.steps, args.kernel_iters, "kernel")
                        x.update({"net": name, "batch": batch, "round": r, "leg": kind, "lib": os.path.relpath(engine.LIB_PATH, ROOT)})
                        print(json.dumps(x), flush=True)
                        lines.append(x)
                        res[kind].append(x)
                for eng in engs.values():
                    eng.close()
                med = lambda k, f: sorted(v[f] for v in res[k])[len(res[k]) // 2]
                s = {"summary": True, "net": name, "batch": batch, "rounds": args.rounds, "steps": args.steps,
                     "lib": os.path.relpath(engine.LIB_PATH, ROOT)}
                for kind in engs:
                    ms = [v["ms_per_forward"] for v in res[kind]]
                    s[kind + "_pos_per_s"] = med(kind, "pos_per_s")
                    s[kind + "_ms_per_forward"] = med(kind, "ms_per_forward")
                    s[kind + "_spread"] = (max(ms) - min(ms)) / s[kind + "_ms_per_forward"]
                    s[kind + "_kernel"] = res[kind][0]["kernel_name"]
                    s[kind + "_kernel_ms"] = med(kind, "kernel_ms")
                    chips = [v["chip"] for v in res[kind] if v.get("chip")]
                    if chips:
                        s[kind + "_chip"] = chips[len(chips) // 2]
                if len(engs) == 2:
                    s["aux_over_plain_time"] = s["aux_ms_per_forward"] / s["plain_ms_per_forward"]
                    s["aux_extra_ms_per_forward"] = s["aux_ms_per_forward"] - s["plain_ms_per_forward"]
                print(json.dumps(s), flush=True)
                lines.append(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
