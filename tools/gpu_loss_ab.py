"""The validation losses computed on the device against fetching every output and computing them on the host,
interleaved A/B on one MI355X: b12c256btl3 + P3HIP_FLAG_AUX at batch 1024 by default.  The twin of the
profiles/dataset_score_ab.jsonl measurement (tools/dataset_benchmark.py --ab).

Both legs walk the same batches of one chunk on one engine: LoadBatch + targets, RunInference, then
  device   p3hip_loss: the targets go up, k_loss_rows + k_loss_sum run behind the forward pass, 19 sums and the term rows
           come back;
  host     per position p3hip_get_raw + p3hip_get_aux, then dataset.host_loss_terms (vectorised numpy, float64) and a sum.
Legs alternate device, host, device, host, ... for --reps rounds after a warm-up; every time is a host clock around calls
that end in a stream synchronise.  Reported per leg: seconds in load, run and loss, microseconds of the loss step per
batch, positions/s over run + loss; the record holds the medians over the rounds and whether the two legs' sums agree
(rtol 1e-5: the device rounds each term to float once).

The chunk: CHUNK arguments, or --games copies of the scripted game of tests/dataset_common.py recorded through the host's
recorder into a temporary directory (every record has targets).  Weights are random-init unless WEIGHTS is a .p3w: the
timing is real, the losses mean nothing.  Appends one JSON line to profiles/loss_ab.jsonl.

  python tools/gpu_loss_ab.py [WEIGHTS] [CHUNK...] [--batch 1024] [--reps 3] [--games 410] [--warmup 10] [--out FILE]
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

from p3achygo_amd import dataset, engine, netspec  # noqa: E402


def host_loss(eng, targets):
    """(sums, n) like HipEngine.loss(), through the fetch path."""
    n = len(targets)
    raw, aux = np.zeros((n, engine.RAW_LEN), np.float32), np.zeros((n, engine.AUX_LEN), np.float32)
    for i in range(n):
        raw[i], aux[i] = eng.get_raw(i), eng.GetAux(i)
    return dataset.host_loss_terms(raw, aux, targets).sum(axis=0), n


def run_leg(eng, batch_list, host):
    total = np.zeros(engine.NUM_LOSS_TERMS, np.float64)
    count = prev = 0
    t_load = t_run = t_loss = 0.0
    for feats, _, targets, has in batch_list:
        t0 = time.perf_counter()
        prev = dataset.load_batch(eng, feats, None, prev, targets, has)
        t1 = time.perf_counter()
        eng.RunInference()
        t2 = time.perf_counter()
        sums, n = host_loss(eng, targets) if host else eng.loss()
        t3 = time.perf_counter()
        total += sums
        count += n
        t_load += t1 - t0
        t_run += t2 - t1
        t_loss += t3 - t2
    dataset.release(eng, 0, prev)
    nb = max(len(batch_list), 1)
    return total, {"load_s": t_load, "run_s": t_run, "loss_s": t_loss, "batches": len(batch_list), "positions": count,
                   "run_us_per_batch": t_run / nb * 1e6, "loss_us_per_batch": t_loss / nb * 1e6,
                   "positions_per_s_run_and_loss": count / max(t_run + t_loss, 1e-12)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("weights", nargs="?", default="b12c256btl3")
    ap.add_argument("chunks", nargs="*")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--games", type=int, default=410)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_ab.jsonl"))
    args = ap.parse_args(argv)

    tmp = tempfile.mkdtemp()
    random_init = not os.path.isfile(args.weights)
    if random_init:
        cfg = netspec.CONFIGS[args.weights]
        path = os.path.join(tmp, args.weights + ".p3w")
        netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
    else:
        path = args.weights
    chunks = args.chunks
    if not chunks:
        import dataset_common as dc
        os.makedirs(os.path.join(tmp, "chunk"))
        chunks = [dc.record_game(os.path.join(tmp, "chunk"), games=args.games)]
    batch_list = [b for b in dataset.batches(chunks, args.batch, with_targets=True) if b[3].all()]
    if not batch_list:
        sys.exit("the chunks hold no batch whose records all have targets")
    full = [b for b in batch_list if len(b[0]) == args.batch]
    batch_list = full or batch_list   # a short last batch would dilute the per-batch times
    eng = engine.HipEngine(path, args.batch, flags=engine.FLAG_AUX)
    prev = dataset.load_batch(eng, batch_list[0][0], None, 0, batch_list[0][2])
    for _ in range(args.warmup):
        eng.RunInference()
        eng.loss()
    dataset.release(eng, 0, prev)
    legs = {"device": [], "host": []}
    sums = {}
    for _ in range(args.reps):
        for name in ("device", "host"):
            sums[name], rec = run_leg(eng, batch_list, name == "host")
            legs[name].append(rec)
            print(json.dumps(dict(rec, leg=name)))
    eng.close()
    med = lambda name, key: float(np.median([r[key] for r in legs[name]]))   # noqa: E731
    rec = {"net": os.path.basename(args.weights), "random_init": random_init, "flags": engine.FLAG_AUX, "batch": args.batch,
           "chunks": [os.path.basename(c) for c in chunks], "reps": args.reps, "positions": legs["device"][0]["positions"],
           "batches": len(batch_list),
           "device_positions_per_s": med("device", "positions_per_s_run_and_loss"),
           "host_positions_per_s": med("host", "positions_per_s_run_and_loss"),
           "p3hip_loss_us_per_batch": med("device", "loss_us_per_batch"),
           "host_loss_us_per_batch": med("host", "loss_us_per_batch"), "run_us_per_batch": med("device", "run_us_per_batch"),
           "p3hip_loss_is": "pinned targets H2D (4,624 B per position), k_loss_rows, k_loss_sum, terms and sums D2H, sync",
           "host_loss_is": "a Python loop of p3hip_get_raw + p3hip_get_aux per position, then dataset.host_loss_terms (numpy)",
           "sums_agree": bool(np.allclose(sums["device"], sums["host"], rtol=1e-5, atol=1e-6)), "legs": legs}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(f"device {rec['device_positions_per_s']:,.0f} positions/s, host {rec['host_positions_per_s']:,.0f} positions/s (run + loss); "
          f"p3hip_loss alone {rec['p3hip_loss_us_per_batch']:.0f} us per batch = "
          f"{100 * rec['p3hip_loss_us_per_batch'] / rec['run_us_per_batch']:.1f} % of the {rec['run_us_per_batch']:.0f} us run; "
          f"host path {rec['host_loss_us_per_batch']:.0f} us per batch; sums agree: {rec['sums_agree']}")


if __name__ == "__main__":
    main()
