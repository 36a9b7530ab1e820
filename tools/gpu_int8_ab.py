"""fp16 against calibrated INT8, interleaved A/B on one MI355X: the layer-wise trunks (P3HIP_FLAG_INT8, the default)
or, with --flag int8_fused, the C = 256 btl trunks (P3HIP_FLAG_INT8_FUSED; default net b12c256btl3), or, with
--flag int8_c128, the C = 128 btl trunks (P3HIP_FLAG_INT8_C128; default net b12c128btl3).

For each trunk and batch size, the two engines are built from the same seeded .p3w; the INT8 engine is calibrated on
tests/int8_restatement.calibration_batches().  Legs alternate fp16, int8, fp16, int8, ...; each leg times
`--steps` device-resident forward passes (engine only: no H2D / D2H) with the chip's clock, power and limiter residency
sampled beside it (p3achygo_amd/power_sampler.py, as bench.py does), then the trunk kernel alone
(p3hip_time_trunk_kernel: the 3x3 layer conv, keys k3x3_*; with --flag int8_fused or int8_c128 the block launch, keys
block_*).
Prints one JSON line per leg and a summary per (trunk, batch); --out writes them all.

  python tools/gpu_int8_ab.py --nets b14c384btl3 b10c384nbt b15c192_classic --batches 1024 256 --rounds 3
  python tools/gpu_int8_ab.py --flag int8_fused --batches 1024 256 --rounds 3 --out profiles/int8_fused_ab.jsonl
  python tools/gpu_int8_ab.py --flag int8_c128 --batches 1024 256 --rounds 3 --out profiles/int8_c128_ab.jsonl
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

# peak dense matrix rates of the MI355X (MI355X_MICROARCH.md: BF16/F16 ~2.5 PF; I8 at twice the BF16 rate)
PEAK_F16 = 2.5e15
PEAK_I8 = 5.0e15


def leg(eng, batch, steps, kernel_iters, k="k3x3"):
    from p3achygo_amd.power_sampler import PowerSampler
    for _ in range(3):
        eng.forward_resident(batch)
    eng.sync()
    try:
        sampler = PowerSampler(0)
        sampler.start()
    except Exception:   # noqa: BLE001
        sampler = None
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.forward_resident(batch)
    eng.sync()
    dt = time.perf_counter() - t0
    power = sampler.stop() if sampler is not None else None
    ms, flops, kname = eng.time_trunk_kernel(batch, kernel_iters)
    return {"pos_per_s": batch * steps / dt, "ms_per_forward": dt / steps * 1e3, k + "_ms": ms, k + "_name": kname,
            k + "_flops": flops, "chip": power}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flag", choices=["int8", "int8_fused", "int8_c128"], default="int8")
    ap.add_argument("--nets", nargs="+", default=None)
    ap.add_argument("--batches", nargs="+", type=int, default=[1024, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--kernel-iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import int8_restatement as ir
    from p3achygo_amd import engine, features, netspec
    fused = args.flag in ("int8_fused", "int8_c128")   # one int8 block launch per btl block
    default_nets = {"int8": ["b14c384btl3", "b10c384nbt", "b15c192_classic"], "int8_fused": ["b12c256btl3"],
                    "int8_c128": ["b12c128btl3"]}
    nets = args.nets or default_nets[args.flag]
    flag = {"int8": engine.FLAG_INT8, "int8_fused": engine.FLAG_INT8_FUSED, "int8_c128": engine.FLAG_INT8_C128}[args.flag]
    k = "block" if fused else "k3x3"
    lines = []
    with tempfile.TemporaryDirectory() as d:
        for name in nets:
            cfg = netspec.CONFIGS[name]
            path = os.path.join(d, name + ".p3w")
            netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
            for batch in args.batches:
                pos = features.random_positions(batch, seed=7, n_games=max(1, batch // 16))
                fp = engine.HipEngine(path, batch)
                i8 = engine.HipEngine(path, batch, flags=flag)
                for cal in ir.calibration_batches():
                    i8.load_all(cal)
                    i8.int8_calibrate()
                    for i in range(len(cal)):
                        i8.GetBatch(i)
                for eng in (fp, i8):
                    eng.load_all(pos)
                    eng.upload()
                res = {"fp16": [], "int8": []}
                for r in range(args.rounds):
                    for kind, eng in (("fp16", fp), ("int8", i8)):
                        x = leg(eng, batch, args.steps, args.kernel_iters, k)
                        x.update({"net": name, "batch": batch, "round": r, "precision": kind, "flag": args.flag})
                        print(json.dumps(x), flush=True)
                        lines.append(x)
                        res[kind].append(x)
                fp.close()
                i8.close()
                med = lambda k, f: sorted(v[f] for v in res[k])[len(res[k]) // 2]
                s = {"summary": True, "net": name, "batch": batch,
                     "fp16_pos_per_s": med("fp16", "pos_per_s"), "int8_pos_per_s": med("int8", "pos_per_s"),
                     "flag": args.flag,
                     f"fp16_{k}_ms": med("fp16", k + "_ms"), f"int8_{k}_ms": med("int8", k + "_ms")}
                s["speedup_forward"] = s["int8_pos_per_s"] / s["fp16_pos_per_s"]
                if not fused:
                    s["speedup_k3x3"] = s["fp16_k3x3_ms"] / s["int8_k3x3_ms"]
                # each leg's own FLOPs per launch: the fp16 block launch covers a run of blocks and the broadcast convs
                # that ride in it, the int8 one a single block
                s[f"fp16_{k}_of_f16_peak"] = res["fp16"][0][k + "_flops"] / (s[f"fp16_{k}_ms"] * 1e-3) / PEAK_F16
                s[f"int8_{k}_of_i8_peak"] = res["int8"][0][k + "_flops"] / (s[f"int8_{k}_ms"] * 1e-3) / PEAK_I8
                if fused:
                    s["fp16_block_flops_per_launch"] = res["fp16"][0]["block_flops"]
                    s["int8_block_flops_per_launch"] = res["int8"][0]["block_flops"]
                for kind in ("fp16", "int8"):
                    chips = [v["chip"] for v in res[kind] if v.get("chip")]
                    if chips:
                        s[kind + "_chip"] = chips[len(chips) // 2]
                print(json.dumps(s), flush=True)
                lines.append(s)
    if args.out:
        with open(args.out, "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
