"""Scores engines on the labelled positions of recorded chunks, in the shape of the reference's nn::Benchmark() +
DefaultStats (cc/nn/engine/benchmark_engine.cc:25-109): a warm-up, then per batch LoadBatch + labels, a timed
RunInference, p3hip_score; at most 1001 batches.  Prints the reference's stats block per plan and appends one JSON line per
plan to profiles/dataset_benchmark.jsonl.

    dataset_benchmark.py WEIGHTS CHUNK... [--batch N] [--plans fp16,fp32,int8] [--calibrate CHUNK...]
                         [--max-batches 1000] [--host-scoring] [--ab REPS] [--loss {rl,sl}]

WEIGHTS is a .p3w file, or the name of a net of p3achygo_amd.netspec.CONFIGS (random-init weights: the timing is real, the
accuracy figures mean nothing; this tool is for trained nets).  Plans: fp16, fp32, int8 (the INT8 plan that serves the
trunk: the shape's own flag, else P3HIP_FLAG_INT8_ANY), or int8_lw / int8_fused / int8_c128 / int8_any / int8_conv3 by name.  INT8
plans are calibrated from the --calibrate chunks through
dataset.calibrate_from_chunks (default: the scored chunks themselves, which flatters them).  --host-scoring scores through
p3hip_get_slot and the numpy restatement (dataset.host_score) instead of p3hip_score.  --ab REPS runs both ways REPS
times, interleaved on one engine, and appends their positions/s and the time of p3hip_score alone to
profiles/dataset_score_ab.jsonl.  --loss rl | sl also prints what the reference's trainer logs for the net, train.py val()
with LossCoeffs.RLCoeffs() or SLCoeffs() (dataset.loss_chunks: the seventeen losses averaged over batches, p3hip_loss on a
P3HIP_FLAG_AUX engine; positions as recorded, no random symmetry, no L2 term), and adds it to the JSON line as "val".

Unlike the reference a short last batch holds only the rows read, and the averages are sums / count rather than running
means.  --warmup, --out and --ab-out only say how many warm-up runs and where the JSON lines go.  Runs on an MI355X; needs
nothing of the reference."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from p3achygo_amd import dataset, engine, netspec  # noqa: E402

PLAN_FLAGS = {"fp16": (0,), "fp32": (engine.FLAG_FP32_ANY,),
              "int8": (engine.FLAG_INT8_FUSED, engine.FLAG_INT8_C128, engine.FLAG_INT8, engine.FLAG_INT8_ANY),
              "int8_lw": (engine.FLAG_INT8,), "int8_fused": (engine.FLAG_INT8_FUSED,), "int8_c128": (engine.FLAG_INT8_C128,),
              "int8_any": (engine.FLAG_INT8_ANY,), "int8_conv3": (engine.FLAG_INT8_CONV3,)}


def create(path, batch, plan, extra=0):
    err = None
    for flags in PLAN_FLAGS[plan]:
        try:
            return engine.HipEngine(path, batch, flags=flags | extra), flags | extra
        except engine.EngineError as e:
            err = e
    raise err


def run_leg(eng, batch_list, host_scoring):
    """One pass over the batches.  Returns the sums, the count and the seconds spent in load, run and scoring."""
    total = np.zeros(engine.NUM_SCORE_TERMS, np.float64)
    count = prev = 0
    t_load = t_run = t_score = 0.0
    for feats, labels in batch_list:
        t0 = time.perf_counter()
        prev = dataset.load_batch(eng, feats, labels, prev)
        t1 = time.perf_counter()
        eng.RunInference()
        t2 = time.perf_counter()
        sums, n = dataset.host_score(eng, labels) if host_scoring else eng.score()
        t3 = time.perf_counter()
        total += sums
        count += n
        t_load += t1 - t0
        t_run += t2 - t1
        t_score += t3 - t2
    dataset.release(eng, 0, prev)
    return total, count, {"load_s": t_load, "run_s": t_run, "score_s": t_score, "batches": len(batch_list)}


def leg_record(count, t):
    return dict(t, positions=count, avg_run_us=t["run_s"] / max(t["batches"], 1) * 1e6,
                avg_score_us=t["score_s"] / max(t["batches"], 1) * 1e6,
                positions_per_s_run_and_score=count / max(t["run_s"] + t["score_s"], 1e-12),
                positions_per_s_with_load=count / max(t["load_s"] + t["run_s"] + t["score_s"], 1e-12))


def append(path, rec):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        f.write(json.dumps(rec) + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("weights")
    ap.add_argument("chunks", nargs="+")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--plans", default="fp16")
    ap.add_argument("--calibrate", nargs="+", default=None, metavar="CHUNK")
    ap.add_argument("--max-batches", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=10, help="runs of the first batch before the clock (the reference: 100)")
    ap.add_argument("--host-scoring", action="store_true")
    ap.add_argument("--ab", type=int, default=0, metavar="REPS")
    ap.add_argument("--loss", choices=("rl", "sl"), default=None, help="also the trainer's validation losses (train.py val())")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_benchmark.jsonl"))
    ap.add_argument("--ab-out", default=os.path.join(ROOT, "profiles", "dataset_score_ab.jsonl"))
    args = ap.parse_args(argv)

    random_init = not os.path.isfile(args.weights)
    if random_init:
        cfg = netspec.CONFIGS[args.weights]
        path = os.path.join(tempfile.mkdtemp(), args.weights + ".p3w")
        netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
        print(f"{args.weights}: random-init weights; the accuracy figures below mean nothing")
    else:
        path = args.weights
    batch_list = list(dataset.batches(args.chunks, args.batch, min(args.max_batches, 1001)))   # benchmark_engine.cc:88
    if not batch_list:
        sys.exit("the chunks hold no positions")
    for plan in args.plans.split(","):
        eng, flags = create(path, args.batch, plan, engine.FLAG_AUX if args.loss else 0)
        common = {"net": os.path.basename(args.weights), "random_init": random_init, "plan": plan, "flags": flags,
                  "batch": args.batch, "chunks": [os.path.basename(c) for c in args.chunks]}
        if plan.startswith("int8"):
            cal = args.calibrate or args.chunks
            if not args.calibrate:
                print("int8: no --calibrate chunks, calibrating on the scored chunks themselves")
            common["calibration_batches"] = dataset.calibrate_from_chunks(eng, cal, args.max_batches)
        prev = dataset.load_batch(eng, batch_list[0][0])
        for _ in range(args.warmup):
            eng.RunInference()
        dataset.release(eng, 0, prev)
        if args.ab > 0:
            legs = {"device": [], "host": []}
            sums = {}
            for _ in range(args.ab):
                for name in ("device", "host"):
                    total, count, t = run_leg(eng, batch_list, name == "host")
                    legs[name].append(leg_record(count, t))
                    sums[name] = total
            med = lambda name, key: float(np.median([r[key] for r in legs[name]]))   # noqa: E731
            rec = dict(common, reps=args.ab, positions=legs["device"][0]["positions"],
                       device_positions_per_s=med("device", "positions_per_s_run_and_score"),
                       host_positions_per_s=med("host", "positions_per_s_run_and_score"),
                       p3hip_score_us_per_batch=med("device", "avg_score_us"),
                       host_scoring_us_per_batch=med("host", "avg_score_us"), run_us_per_batch=med("device", "avg_run_us"),
                       host_scoring_is="a Python loop of p3hip_get_slot plus numpy", legs=legs,
                       sums_agree=bool(np.allclose(sums["device"], sums["host"], rtol=1e-6, atol=1e-6)))
            append(args.ab_out, rec)
            print(f"{plan}: device scoring {rec['device_positions_per_s']:,.0f} positions/s, host scoring "
                  f"{rec['host_positions_per_s']:,.0f} positions/s (run + scoring; p3hip_score alone "
                  f"{rec['p3hip_score_us_per_batch']:.0f} us per batch, host scoring {rec['host_scoring_us_per_batch']:.0f} us)")
        total, count, t = run_leg(eng, batch_list, args.host_scoring)
        st = dataset.stats_from_sums(total, count)
        print(f"\n{plan} ({'host' if args.host_scoring else 'device'} scoring, {count} positions, {t['batches']} batches)"
              "\nStats:"
              f"\n  Avg Inference Time: {t['run_s'] / t['batches'] * 1e6:.6g}us"
              f"\n  Avg Policy Loss: {st['policy_loss']:.6g}"
              f"\n  Avg Outcome Loss: {st['outcome_loss']:.6g}"
              f"\n  Correct Move Percentage: {st['policy_percent']:.6g}"
              f"\n  Correct Outcome Percentage: {st['outcome_percent']:.6g}"
              f"\n  Mean Score Diff: {st['score_diff']:.6g}")
        rec = dict(common, scoring="host" if args.host_scoring else "device", stats=st, **leg_record(count, t))
        if args.loss:
            coeffs = dataset.LossCoeffs.rl() if args.loss == "rl" else dataset.LossCoeffs.sl()
            val = dataset.loss_chunks(eng, args.chunks, coeffs, min(args.max_batches, 1001))
            print(f"Validation losses ({args.loss} coefficients, {val['positions']} positions, {val['batches']} batches; as "
                  "recorded: no symmetry, no L2 term):")
            for k in dataset.LOSS_NAMES:
                print(f"  {k}: {val[k]:.6g}")
            print(f"  move accuracy: {val['move_accuracy']:.6g}\n  outcome accuracy: {val['outcome_accuracy']:.6g}")
            rec["val"] = dict(val, coeffs=args.loss)
        append(args.out, rec)
        eng.close()


if __name__ == "__main__":
    main()
