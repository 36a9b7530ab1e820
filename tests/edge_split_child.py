"""The child process of tests/test_edge_split_gpu.py: engines whose P3HIP_* environment differs from the test's own.

    python tests/edge_split_child.py OUT.npz JOBS.json

JOBS is a list of jobs; a job is a dict
    key      name of its results in OUT
    path     the .p3w
    batch    the static batch
    flags    engine flags
    env      {variable: value} set for p3hip_create (P3HIP_EDGE_SPLIT and P3HIP_DEBUG_STOP_BLOCK are cleared first)
    loads    one list of slots per run (default: one run of every slot); slot s holds position s % mod of
             features.random_positions(16, seed=43)
    mod      default 16
    sym      symmetry mask set before the first run (FLAG_SYMMETRY_AVG engines), or absent
    x        channels: also read the residual stream after the last run (debug_x), or absent
    aux      true: also read the aux records of the last run
and leaves, per run r, OUT[key:r] = [loaded slot][raw floats | result record | ownership] as uint32, OUT[key:g] = the
graph state after every run, and OUT[key:x], OUT[key:aux] where asked for.

TEST INFRASTRUCTURE ONLY."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    from p3achygo_amd import engine, features
    outp, jobs = sys.argv[1], json.load(open(sys.argv[2]))
    pos = features.random_positions(16, seed=43)
    out = {}
    for job in jobs:
        for v in ("P3HIP_EDGE_SPLIT", "P3HIP_DEBUG_STOP_BLOCK"):
            os.environ.pop(v, None)
        os.environ.update(job.get("env", {}))
        batch, key, mod = job["batch"], job["key"], job.get("mod", 16)
        eng = engine.HipEngine(job["path"], batch, flags=job["flags"])
        if job.get("sym"):
            eng.set_symmetries(job["sym"])
        states = []
        for r, slots in enumerate(job.get("loads") or [list(range(batch))]):
            for s in slots:
                eng.LoadBatch(s, pos[s % mod:s % mod + 1])
            eng.RunInference()
            states.append(eng.graph_state())
            rows = []
            for s in slots:
                res = np.frombuffer(bytes(eng.GetBatch(s)), np.uint32)
                rows.append(np.concatenate([eng.get_raw(s).view(np.uint32), res, eng.GetOwnership(s).view(np.uint32)]))
            out["%s:%d" % (key, r)] = np.stack(rows)
        out[key + ":g"] = np.array(states)
        if job.get("x"):
            out[key + ":x"] = eng.debug_x(batch, job["x"])
        if job.get("aux"):
            out[key + ":aux"] = np.stack([eng.GetAux(s) for s in range(batch)])
        eng.close()
    np.savez(outp, **out)


if __name__ == "__main__":
    main()
