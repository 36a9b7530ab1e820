"""Engine-only throughput of conv trunks of the widths csrc/conv_any.hip serves: positions/s of the resident forward
pass at batch 1024 and the whole-net share of the 2.5 PFLOP/s fp16 peak (the file's own, unpadded FLOPs over time: a
whole-net figure, stem, broadcast blocks and heads included), for each of a list of netspec configs, and the templated
layer-wise kernels against the runtime-width ones on b14c384btl3 (P3HIP_CONV_ANY=1, read when an engine is created),
the two paths interleaved round by round.  Appends one JSON line per measurement to profiles/conv_widths_bench.jsonl.

    python tools/gpu_conv_widths_bench.py [seconds per measurement] [config ...]

Per-kernel shares come from a run of its own under rocprofv3 (the program after `--`):
    rocprofv3 --kernel-trace --stats -d DIR -o conv_any -- python tools/gpu_conv_widths_bench.py 1 b10c512nbt
"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from p3achygo_amd import engine, features, netspec  # noqa: E402

PEAK = 2.5e15
BATCH = 1024
OUT = os.path.join(ROOT, "profiles", "conv_widths_bench.jsonl")
secs = float(sys.argv[1]) if len(sys.argv) > 1 else 3.0
names = sys.argv[2:] or ["b12c192btl3", "b10c512nbt", "b14c320btl3", "b14c384btl3"]
AB = "b14c384btl3"   # runs on either path


def make_engine(path, any_path):
    if any_path:
        os.environ["P3HIP_CONV_ANY"] = "1"
    else:
        os.environ.pop("P3HIP_CONV_ANY", None)
    eng = engine.HipEngine(path, BATCH)
    os.environ.pop("P3HIP_CONV_ANY", None)
    pos = np.tile(features.random_positions(64, seed=1, n_games=16), BATCH // 64).copy()
    eng.load_all(pos)
    eng.upload()
    for _ in range(10):
        eng.forward_resident(BATCH)
    eng.sync()
    return eng


def measure(eng, seconds):
    """(forward passes, seconds) of at least `seconds` of resident forward passes"""
    t0 = time.perf_counter()
    n = 0
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            eng.forward_resident(BATCH)
        eng.sync()
        n += 10
    return n, time.perf_counter() - t0


def record(cfg, path_name, eng, n, dt):
    total, _ = eng.flops_per_position()
    ms, fl, kname = eng.time_trunk_kernel(BATCH, 3)
    row = {"net": cfg.name, "path": path_name, "batch": BATCH, "forward_ms": dt / n * 1e3,
           "positions_per_s": BATCH * n / dt, "whole_net_tflops": BATCH * n / dt * total / 1e12,
           "whole_net_share_of_peak": BATCH * n / dt * total / PEAK, "kernel": kname, "kernel_us": ms * 1e3,
           "kernel_tflops": fl / ms / 1e9}
    print(json.dumps(row), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")
    return row


for name in names:
    cfg = netspec.get_config(name)
    path = os.path.join(tempfile.mkdtemp(), name + ".p3w")
    netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
    if name != AB:
        eng = make_engine(path, False)
        record(cfg, "conv_any", eng, *measure(eng, secs))
        eng.close()
        continue
    # both paths alive at once, measured in alternating rounds so that clock and power drift hit both alike
    engs = {"templated": make_engine(path, False), "conv_any": make_engine(path, True)}
    tot = {k: [0, 0.0] for k in engs}
    for _ in range(4):
        for k, eng in engs.items():
            n, dt = measure(eng, secs / 4)
            tot[k][0] += n
            tot[k][1] += dt
    rows = {k: record(cfg, k, engs[k], *tot[k]) for k in engs}
    ratio = rows["conv_any"]["forward_ms"] / rows["templated"]["forward_ms"]
    row = {"net": cfg.name, "conv_any_over_templated_forward_time": ratio}
    print(json.dumps(row), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(row) + "\n")
    for eng in engs.values():
        eng.close()
