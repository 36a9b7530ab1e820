"""Engine-only throughput of transformer trunks: positions/s of the resident forward pass at batch 256 and 1024, the
whole-net FLOP rate, the per-launch time of the attention kernel and its share of the pass, and the chip state while it
runs, for each of a list of configs.

    python tools/gpu_transformer_bench.py [seconds per batch size] [config ...]

A config is a netspec name (b14d96h3_transformer, the default) or dDhH: 14 blocks of model width D with H heads (e.g.
d256h8).  Per-kernel times (every kernel's share of the pass) come from a run of its own under rocprofv3 (the program
after `--`):
    rocprofv3 --kernel-trace --stats -d DIR -o tfm -- python tools/gpu_transformer_bench.py 1 d256h8
"""
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from p3achygo_amd import engine, features, netspec  # noqa: E402

secs = float(sys.argv[1]) if len(sys.argv) > 1 else 3.0
names = sys.argv[2:] or ["b14d96h3_transformer"]
try:
    from p3achygo_amd.power_sampler import PowerSampler
    smp = PowerSampler(0)
except Exception:   # no sampler on this box: throughput only
    smp = None


def config(name):
    m = re.fullmatch(r"d(\d+)h(\d+)", name)
    if m:
        return netspec.transformer_config(f"b14{name}_transformer", 14, int(m.group(1)), int(m.group(2)))
    return netspec.get_config(name)


for name in names:
    cfg = config(name)
    path = os.path.join(tempfile.mkdtemp(), "tfm.p3w")
    netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
    for batch in (256, 1024):
        pos = np.tile(features.random_positions(64, seed=1, n_games=16), batch // 64).copy()
        eng = engine.HipEngine(path, batch)
        eng.load_all(pos)
        eng.upload()
        for _ in range(20):
            eng.forward_resident(batch)
        eng.sync()
        if smp:
            smp.start()
        t0 = time.perf_counter()
        n = 0
        while time.perf_counter() - t0 < secs:
            for _ in range(20):
                eng.forward_resident(batch)
            eng.sync()
            n += 20
        dt = time.perf_counter() - t0
        st = (smp.stop() if smp else None) or {}
        total, _ = eng.flops_per_position()
        ms, fl, kname = eng.time_trunk_kernel(batch, 5)
        fwd_ms = dt / n * 1e3
        print(f"{cfg.name} batch {batch:5d}  forward {fwd_ms:7.3f} ms  {batch * n / dt / 1e3:7.1f} k positions/s  "
              f"{batch * n / dt * total / 1e12:6.1f} TFLOP/s whole net  {kname} {ms * 1e3:7.1f} us/launch "
              f"({fl / ms / 1e9:5.1f} TFLOP/s, {100 * ms * cfg.blocks / fwd_ms:4.1f} % of the pass)  "
              f"clock {st.get('gfx_clock_mhz_mean', 0):5.0f} MHz  power {st.get('socket_power_w_mean', 0):5.0f} W",
              flush=True)
        eng.close()
