"""fp16 against fp32 (P3HIP_FLAG_FP32_ANY: P3HIP_FLAG_FP32 on conv trunks, P3HIP_FLAG_FP32_TFM on transformers),
interleaved A/B on one MI355X.

For each trunk and batch size, the two engines are built from the same seeded .p3w.  Legs alternate fp16, fp32, fp16,
fp32, ...; each leg times `--steps` device-resident forward passes (engine only: no H2D / D2H) with the chip's clock,
power and limiter residency sampled beside it (p3achygo_amd/power_sampler.py, as bench.py does), then the trunk kernel
alone (p3hip_time_trunk_kernel).  The fp32 leg's kernel is the 3x3 layer conv k_lconv_f32<3>, reported with its time per
launch and its fraction of the 157.3 TFLOP/s of the f32-input MFMA; the fp16 leg's is whatever the fp16 plan of the
trunk runs (the fused block kernel at C = 128 / 256, the 3x3 layer conv at C = 384).  On a transformer trunk both legs
time their attention kernel (k_tfm_attn, k_tfm_attn_f32), and the summary's fp32 kernel keys are fp32_attn_* where a conv
trunk has fp32_k3x3_*.
Prints one JSON line per leg and a summary per (trunk, batch); --out writes them all.

  python tools/gpu_fp32_ab.py --out profiles/fp32_ab.jsonl
  python tools/gpu_fp32_ab.py --nets test_b2d96h3_tfm test_b2d192h6_tfm test_b2d384h12_tfm --batches 1024 \
      --out profiles/fp32_tfm_ab.jsonl
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PEAK_F32_MFMA = 157.3e12   # v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32: the fp32 vector rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="+", default=["b12c256btl3", "b12c128btl3", "b14c384btl3"])
    ap.add_argument("--batches", nargs="+", type=int, default=[256, 1024])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
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
                engs = {"fp16": engine.HipEngine(path, batch), "fp32": engine.HipEngine(path, batch, flags=engine.FLAG_FP32_ANY)}
                for eng in engs.values():
                    eng.load_all(pos)
                    eng.upload()
                res = {"fp16": [], "fp32": []}
                for r in range(args.rounds):
                    for kind, eng in engs.items():
                        x = leg(eng, batch, args.steps, args.kernel_iters, "kernel")
                        x.update({"net": name, "batch": batch, "round": r, "precision": kind})
                        print(json.dumps(x), flush=True)
                        lines.append(x)
                        res[kind].append(x)
                for eng in engs.values():
                    eng.close()
                med = lambda k, f: sorted(v[f] for v in res[k])[len(res[k]) // 2]
                k32 = "fp32_attn" if cfg.block_type == "transformer" else "fp32_k3x3"
                s = {"summary": True, "net": name, "batch": batch,
                     "fp16_pos_per_s": med("fp16", "pos_per_s"), "fp32_pos_per_s": med("fp32", "pos_per_s"),
                     "fp16_kernel": res["fp16"][0]["kernel_name"], "fp16_kernel_ms": med("fp16", "kernel_ms"),
                     "fp32_kernel": res["fp32"][0]["kernel_name"], k32 + "_ms": med("fp32", "kernel_ms")}
                s["fp32_over_fp16_time"] = s["fp16_pos_per_s"] / s["fp32_pos_per_s"]
                s[k32 + "_tflops"] = res["fp32"][0]["kernel_flops"] / (s[k32 + "_ms"] * 1e-3) / 1e12
                s[k32 + "_of_f32_mfma_peak"] = s[k32 + "_tflops"] * 1e12 / PEAK_F32_MFMA
                for kind in ("fp16", "fp32"):
                    chips = [v["chip"] for v in res[kind] if v.get("chip")]
                    if chips:
                        s[kind + "_chip"] = chips[len(chips) // 2]
                print(json.dumps(s), flush=True)
                lines.append(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
