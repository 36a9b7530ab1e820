"""fp16 against calibrated INT8 on the layer-wise trunks, interleaved A/B on one MI355X (P3HIP_FLAG_INT8).

For each trunk and batch size, the two engines are built from the same seeded .p3w; the INT8 engine is calibrated on
tests/int8_restatement.calibration_batches().  Legs alternate fp16, int8, fp16, int8, ...; each leg times
`--steps` device-resident forward passes (engine only: no H2D / D2H) with the chip's clock, power and limiter residency
sampled beside it (p3achygo_amd/power_sampler.py, as bench.py does), then the 3x3 layer conv alone
(p3hip_time_trunk_kernel).  Prints one JSON line per leg and a summary per (trunk, batch); --out writes them all.

  python tools/gpu_int8_ab.py --nets b14c384btl3 b10c384nbt b15c192_classic --batches 1024 256 --rounds 3
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


def leg(eng, batch, steps, kernel_iters):
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
    return {"pos_per_s": batch * steps / dt, "ms_per_forward": dt / steps * 1e3, "k3x3_ms": ms, "k3x3_name": kname,
            "k3x3_flops": flops, "chip": power}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="+", default=["b14c384btl3", "b10c384nbt", "b15c192_classic"])
    ap.add_argument("--batches", nargs="+", type=int, default=[1024, 256])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--kernel-iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import int8_restatement as ir
    from p3achygo_amd import engine, features, netspec
    lines = []
    with tempfile.TemporaryDirectory() as d:
        for name in args.nets:
            cfg = netspec.CONFIGS[name]
            path = os.path.join(d, name + ".p3w")
            netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
            for batch in args.batches:
                pos = features.random_positions(batch, seed=7, n_games=max(1, batch // 16))
                fp = engine.HipEngine(path, batch)
                i8 = engine.HipEngine(path, batch, flags=engine.FLAG_INT8)
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
                        x = leg(eng, batch, args.steps, args.kernel_iters)
                        x.update({"net": name, "batch": batch, "round": r, "precision": kind})
                        print(json.dumps(x), flush=True)
                        lines.append(x)
                        res[kind].append(x)
                fp.close()
                i8.close()
                med = lambda k, f: sorted(v[f] for v in res[k])[len(res[k]) // 2]
                s = {"summary": True, "net": name, "batch": batch,
                     "fp16_pos_per_s": med("fp16", "pos_per_s"), "int8_pos_per_s": med("int8", "pos_per_s"),
                     "fp16_k3x3_ms": med("fp16", "k3x3_ms"), "int8_k3x3_ms": med("int8", "k3x3_ms")}
                fl = res["int8"][0]["k3x3_flops"]
                s["speedup_forward"] = s["int8_pos_per_s"] / s["fp16_pos_per_s"]
                s["speedup_k3x3"] = s["fp16_k3x3_ms"] / s["int8_k3x3_ms"]
                s["fp16_k3x3_of_f16_peak"] = fl / (s["fp16_k3x3_ms"] * 1e-3) / PEAK_F16
                s["int8_k3x3_of_i8_peak"] = fl / (s["int8_k3x3_ms"] * 1e-3) / PEAK_I8
                print(json.dumps(s), flush=True)
                lines.append(s)
    if args.out:
        with open(args.out, "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
