"""What each precision plan costs in accuracy, measured against the fp32 engine on one MI355X: the counterpart of the
reference's cc/nn/engine/scripts/compare_engines.cc.

For one net and N positions of features.random_positions, runs the fp32 engine (P3HIP_FLAG_FP32_ANY: the fp32 plan of
the net's trunk, conv or transformer; a transformer's only other plan is fp16), the fp16 engine and
every INT8 plan that serves the net (P3HIP_FLAG_INT8, _INT8_FUSED, _INT8_C128: the ones p3hip_create accepts, calibrated
on the same positions; where none of the three does, P3HIP_FLAG_INT8_ANY's own layer-wise plan, row "int8_any"; P3HIP_FLAG_INT8_CONV3 where it
has a plan of its own, row "int8_conv3"; P3HIP_FLAG_WINOGRAD where it serves the net, row "winograd", uncalibrated), and prints one JSON line per plan: its largest and mean deviation from the fp32 engine in the raw
outputs and in the move, value and score probabilities, and the largest and mean KL(fp32 || plan) of the move, value and
score distributions.  --out writes the lines (default profiles/precision_report.jsonl); --append adds them to the file.

  python tools/gpu_precision_report.py --net b12c256btl3 --positions 1024
  python tools/gpu_precision_report.py --net b14d96h3_transformer --positions 512 --append
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("move_probs", "value_probs", "score_probs")


def evaluate(eng, pos, batch):
    """raw [n, 1889] and the three distributions of every position, `batch` at a time"""
    out = {k: [] for k in ("raw",) + KEYS}
    for i in range(0, len(pos), batch):
        part = pos[i:i + batch]
        eng.load_all(part)
        eng.RunInference()
        for s in range(len(part)):
            out["raw"].append(eng.get_raw(s).copy())
            r = eng.GetBatch(s)
            for k in KEYS:
                out[k].append(np.ctypeslib.as_array(getattr(r, k)).copy())
    return {k: np.stack(v).astype(np.float64) for k, v in out.items()}


def kl(p, q):
    q = np.maximum(q, 1e-30)
    return np.where(p > 0, p * (np.log(np.maximum(p, 1e-300)) - np.log(q)), 0.0).sum(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="b12c256btl3")
    ap.add_argument("--positions", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precision_report.jsonl"))
    ap.add_argument("--append", action="store_true", help="add the lines to --out instead of replacing it")
    args = ap.parse_args()
    from p3achygo_amd import engine, features, netspec
    cfg = netspec.get_config(args.net)
    pos = features.random_positions(args.positions, seed=args.seed, n_games=max(1, args.positions // 16))
    lines = []
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, args.net + ".p3w")
        netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
        eng = engine.HipEngine(path, args.batch, flags=engine.FLAG_FP32_ANY)
        ref = evaluate(eng, pos, args.batch)
        eng.close()
        plans = [("fp16", 0), ("int8", engine.FLAG_INT8), ("int8_fused", engine.FLAG_INT8_FUSED), ("int8_c128", engine.FLAG_INT8_C128),
                 ("int8_any", engine.FLAG_INT8_ANY), ("int8_conv3", engine.FLAG_INT8_CONV3),
                 ("winograd", engine.FLAG_WINOGRAD)]
        for label, flag in plans:
            # (on a trunk one of the three other INT8 flags serves, INT8_ANY is that flag's plan bit for bit: no second row)
            if label == "int8_any" and any(x["plan"].startswith("int8") for x in lines):
                continue
            # (P3HIP_FLAG_INT8_CONV3: a row where the flag has a plan of its own; a classic trunk's is the int8 row's)
            if label == "int8_conv3":
                try:
                    if engine.debug_plan(path, flag)[0] != "Int8Conv3":
                        continue
                except engine.EngineError:
                    continue
            try:
                eng = engine.HipEngine(path, args.batch, flags=flag)
            except engine.EngineError:
                continue   # the plan does not serve this net
            if flag and label != "winograd":   # (P3HIP_FLAG_WINOGRAD needs no calibration)
                for i in range(0, len(pos), args.batch):
                    part = pos[i:i + args.batch]
                    eng.load_all(part)
                    eng.int8_calibrate()
                    for s in range(len(part)):
                        eng.GetBatch(s)
            got = evaluate(eng, pos, args.batch)
            eng.close()
            x = {"net": args.net, "positions": len(pos), "plan": label, "reference": "fp32"}
            for k in ("raw",) + KEYS:
                dlt = np.abs(got[k] - ref[k])
                x[k + "_max"], x[k + "_mean"] = float(dlt.max()), float(dlt.mean())
            for k in KEYS:
                v = kl(ref[k], got[k])
                x[k + "_kl_max"], x[k + "_kl_mean"] = float(v.max()), float(v.mean())
            print(json.dumps(x), flush=True)
            lines.append(x)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
