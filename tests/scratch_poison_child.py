"""The child process of tests/test_scratch_poison_gpu.py: one engine at a time, each configuration three times over (never
poisoned, p3hip_debug_poison(0xFF) and p3hip_debug_poison(0x7B) in front of every calibration and every run).

    python tests/scratch_poison_child.py IN.npz OUT.npz JOBS.json

IN holds the position pools ("pool:<id>", feature records as bytes), "labels" and "targets" (one record per pool index)
and "calib:<b>" (the INT8 calibration batches).  JOBS is a list of jobs; a job is a dict
    key      name of its results in OUT
    path     the .p3w
    batch    the static batch
    flags    engine flags
    env      {variable: value} set for p3hip_create (every P3HIP_* variable but P3HIP_LIB is cleared first)
    pool     id of its position pool
    runs     [{"slots": [...], "pos": [pool index per slot], "masks": [per-slot symmetry masks] or absent,
               "avg": mask for set_symmetries or absent}]
    int8     true: calibrate on the calibration batches first (and keep the scales)
    cache    log2 of the NN cache's entries, or absent; slots are then loaded with key (pool index + 1, 7)
    labels   true: labels and targets are loaded with every slot, score() and loss() read after every run
    tfm      [heads, head width] of a transformer without symmetries: after every run q, k and v are read back and
             whether their token rows 361..383 are exactly zero is kept
and leaves, per mode m in ("clean", "ff", "7b") and run r, OUT[key:m:r:raw|own|rec|aux|hit|score|loss|state|zero] and
OUT[key:m:scales].

TEST INFRASTRUCTURE ONLY."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

MODES = (("clean", None), ("ff", 0xFF), ("7b", 0x7B))


def run_job(engine, job, byte, data, out, prefix):
    pos, labels, targets = data["pool:" + job["pool"]], data["labels"], data["targets"]
    for v in [v for v in os.environ if v.startswith("P3HIP_") and v != "P3HIP_LIB"]:
        del os.environ[v]
    os.environ.update(job.get("env", {}))
    eng = engine.HipEngine(job["path"], job["batch"], flags=job["flags"])

    def poison():
        if byte is not None:
            eng.debug_poison(byte)

    if job.get("cache"):
        eng.EnableCache(job["cache"])
    if job.get("int8"):
        for cal in data["calib"]:
            poison()
            eng.load_all(cal)
            eng.int8_calibrate()
            for i in range(len(cal)):
                eng.GetBatch(i)
        out[prefix + "scales"] = eng.int8_scales()
    aux = bool(job["flags"] & engine.FLAG_AUX)
    for r, run in enumerate(job["runs"]):
        slots = run["slots"]
        poison()
        if run.get("avg"):
            eng.set_symmetries(run["avg"])
        for k, (s, p) in enumerate(zip(slots, run["pos"])):
            if job.get("cache"):
                eng.LoadBatchKeyed(s, pos[p:p + 1], p + 1, 7, 0)
            else:
                eng.LoadBatch(s, pos[p:p + 1])
            if run.get("masks"):
                eng.set_slot_symmetries(s, run["masks"][k])
            if job.get("labels"):
                eng.load_labels(s, labels[p:p + 1])
                eng.load_targets(s, targets[p:p + 1])
        eng.RunInference()
        key = "%s%d:" % (prefix, r)
        out[key + "state"] = np.array([eng.graph_state()])
        out[key + "raw"] = np.stack([eng.get_raw(s) for s in slots])
        out[key + "own"] = np.stack([eng.GetOwnership(s) for s in slots])
        if aux:
            out[key + "aux"] = np.stack([eng.GetAux(s) for s in slots])
        if job.get("labels"):
            sums, n = eng.score()
            out[key + "score"] = np.concatenate([sums, [n]] + [eng.get_score(s).astype(np.float64) for s in slots])
            sums, n = eng.loss()
            out[key + "loss"] = np.concatenate([sums, [n]] + [eng.get_loss(s).astype(np.float64) for s in slots])
        if job.get("tfm"):
            heads, D = job["tfm"]
            out[key + "zero"] = np.array([bool((eng.debug_tfm(w, len(slots), heads, D)[:, :, 361:, :] == 0).all())
                                          for w in range(3)])
        # the result records last: fetching one takes the slot out of the next run
        recs, hits = [], []
        for s in slots:
            if job.get("cache"):
                res, _, hit = eng.GetBatchKeyed(s)
            else:
                res, hit = eng.GetBatch(s), False
            recs.append(np.frombuffer(bytes(res), np.uint8))
            hits.append(hit)
        out[key + "rec"] = np.stack(recs)
        out[key + "hit"] = np.array(hits)
    eng.close()


def main():
    from p3achygo_amd import engine, features
    z = np.load(sys.argv[1])
    data = {k: np.frombuffer(z[k].tobytes(), dtype=features.features_dtype()).copy() for k in z.files if k.startswith("pool:")}
    data["labels"] = np.frombuffer(z["labels"].tobytes(), dtype=engine.labels_dtype()).copy()
    data["targets"] = np.frombuffer(z["targets"].tobytes(), dtype=engine.targets_dtype()).copy()
    data["calib"] = [np.frombuffer(z[k].tobytes(), dtype=features.features_dtype()).copy()
                     for k in sorted(k for k in z.files if k.startswith("calib:"))]
    out = {}
    try:   # (an engine error ends the child there: nothing more is started on the device, what was read is kept)
        for job in json.load(open(sys.argv[3])):
            for mode, byte in MODES:
                run_job(engine, job, byte, data, out, "%s:%s:" % (job["key"], mode))
                print(job["key"], mode, "done", flush=True)
    finally:
        np.savez(sys.argv[2], **out)


if __name__ == "__main__":
    main()
