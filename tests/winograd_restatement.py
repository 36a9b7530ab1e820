"""CPU emulation of the Winograd plan (P3HIP_FLAG_WINOGRAD), its twin, and the thresholds of
tests/test_winograd_cpu.py and tests/test_winograd_gpu.py.

TEST INFRASTRUCTURE ONLY.  `WTrunk` is tests/trunk_emulation.py's Trunk (through conv_widths_common.trunk: every served
net runs layer by layer) with another 3x3 conv: F(2x2, 3x3) Winograd as csrc/conv_wino.hip computes it, operation for
operation at its storage points.

  * A position is 10 x 10 tiles of 2 x 2 outputs.  Tile (ty, tx) reads the 4 x 4 patch d whose corner is the board point
    (2 ty - 1, 2 tx - 1); rows and columns -1, 19 and 20 are zero; the outputs of row and column 19 are dropped.
  * U = G g G^T per (cin, cout) from the file's fp32 weights (not from their fp16 rounding), in float64, rounded ONCE to
    fp16 (conv_wino.h pack_wconv).
  * d is the activated fp16 input (the value Trunk.act stored; with `pre` the kernel rounds mish(bn(x)) to fp16 first).
  * V = B^T d B in TWO fp16 STAGES: t = B^T d down the rows, every element one fp16 add or subtract (rounded once), then
    V = t B along the rows, again one fp16 operation each.  V is stored as fp16 (LDS).  Both stages are exactly
    reproducible: the float64 sum of two fp16 values is exact, and one rounding to fp16 gives what the packed fp16
    instruction gives, so the emulation's V and the engine's are equal bit for bit.
  * M = sum over cin of U V on fp16 MFMAs, fp32 accumulators: float64 here.
  * Y = A^T M A in fp32, down the rows first, ((M0 + M1) + M2) and ((M1 - M2) - M3), then along the rows: float64 here.
  * then the layer's existing epilogue (residual add, BN, mish, fp16 stores): Trunk's own.
1x1 convs, the stem, the broadcast blocks and the heads are Trunk's, the fp16 plan's.

The TWIN (`WTrunk(..., twin=True)`) has the same storage points (U, V and Trunk's) with float32 arithmetic in another
order: the sum over cin as a float32 torch einsum, Y along the rows first and then down them, grouped (M0 + (M1 + M2)),
and Trunk's twin for everything else.  It is a benign stand-in for the GPU.

Thresholds.  BLOCK_BOUNDS are check_block's (max err in fp16 ulps with trunk_emulation's floor, least bit-identical
fraction) for the engine's x after a block against this emulation from the engine's x before it.  Each is the twin's
worst with the margin trunk_emulation.BOUNDS gives its own kinds (1.5 - 2 x the err, and the identical fraction lowered
by 0.05 - 0.07): the twin's summation order is one of many and the GPU's is another.  TWIN is what
`python tests/winograd_restatement.py` measured on the CPU, over NETS on conv_widths_common.positions() and over the
batches of tests/test_winograd_gpu.py (3, 5 and the second-unit batch of a 256-CU device, test_conv_widths_gpu.block_batch's
positions and slots).  WHOLE_NET are three times EMULATED, the emulation's own error to the float64 outputs
(conv_widths_common.outputs(..., fp16=False)), as int8_conv3_restatement.BOUNDS is made.  Neither is taken from the
engine; what one MI355X measured stands beside them once it has run.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_widths_common as cw  # noqa: E402
import trunk_emulation as te  # noqa: E402

F64 = torch.float64

# the nets of the tests, and what each exercises in k_wconv
NETS = ("test_b3c64btl2",        # one K slice
        "test_b3c192btl3",       # padded C_b (96 -> 128)
        "test_b3c96nbt",         # both widths padded, nbt res / dual
        "test_b3c384btl3",       # the templated widths
        "test_b3c384nbt",
        "test_b3c192classic",    # pre, C -> C
        "test_b3c128classic",
        "test_b4c512btl3_i2")    # broadcast blocks in between
TEMPLATED = ("test_b3c384btl3", "test_b3c384nbt")

G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


def config(name):
    from p3achygo_amd import netspec
    return netspec.get_config(name)


def weights(name):
    from p3achygo_amd import netspec
    return netspec.generate_weights(config(name), randomize=True)


def conv3_width(cfg):
    """the width of the net's 3x3 convs, as the file has it"""
    return cfg.channels if cfg.block_type == "classic" else cfg.bottleneck_channels


def transformed_weights(w, fp16=True):
    """U = G g G^T of a 3x3 conv w [3][3][cin][cout] (fp32 from the file), float64 [4][4][cin][cout]; fp16: rounded once"""
    u = np.einsum("ik,klco,jl->ijco", G, np.asarray(w, np.float32).astype(np.float64), G)
    return u.astype(np.float16).astype(np.float64) if fp16 else u


def patches(a):
    """the 4 x 4 input patches of a [N, C, 19, 19]: [N, C, 10, 10, 4, 4], zeros outside the board"""
    p = torch.nn.functional.pad(a, (1, 2, 1, 2))
    return p.unfold(2, 4, 2).unfold(3, 4, 2)


def _bt(d, dim, r16):
    """B^T applied along `dim` (size 4), each element one operation, rounded by r16"""
    d0, d1, d2, d3 = d.unbind(dim)
    return torch.stack([r16(d0 - d2), r16(d1 + d2), r16(d2 - d1), r16(d1 - d3)], dim)


def input_transform(a, fp16=True):
    """V = B^T d B of every patch of a (float64, fp16 values when fp16): down the rows, then along them; two fp16 stages"""
    r16 = (lambda x: x.half().to(F64)) if fp16 else (lambda x: x)
    return _bt(_bt(patches(a.to(F64)), -2, r16), -1, r16)


def output_transform(m, other_order=False):
    """Y = A^T M A of m [N, C, 10, 10, 4, 4] -> [N, C, 19, 19]; other_order: the twin's"""
    def at(x, dim):
        m0, m1, m2, m3 = x.unbind(dim)
        if other_order:
            return torch.stack([m0 + (m1 + m2), m1 - (m2 + m3)], dim)
        return torch.stack([(m0 + m1) + m2, (m1 - m2) - m3], dim)
    y = at(at(m, -1), -2) if other_order else at(at(m, -2), -1)
    n, c = y.shape[:2]
    return y.permute(0, 1, 2, 4, 3, 5).reshape(n, c, 20, 20)[:, :, :19, :19]


def wino_conv(a, w, fp16=True, dt=F64, other_order=False):
    """The 3x3 conv of a [N, cin, 19, 19] with w [3][3][cin][cout] as k_wconv computes it; fp16=False: the unrounded
    algorithm.  dt, other_order: the twin's arithmetic (float32, another order)"""
    v = input_transform(a, fp16).to(dt)
    u = torch.from_numpy(transformed_weights(w, fp16)).to(dt)
    m = torch.einsum("nctuij,ijco->notuij", v, u)
    return output_transform(m, other_order)


class WTrunk(te.Trunk):
    """trunk_emulation.Trunk, layer-wise at every width, with the 3x3 convs of the blocks as k_wconv computes them"""

    def __init__(self, cfg, W, twin=False):
        super().__init__(cfg, W, fp16=True, twin=twin)
        self.layerwise = True

    def conv(self, a, blk, idx):
        w = self.W[f"blocks.{blk}.conv{idx}.w"]
        if w.shape[0] != 3:
            return super().conv(a, blk, idx)
        return wino_conv(a, w, True, self.dt, self.twin)


def kind_of(cfg, k):
    """the BLOCK_BOUNDS key of block k"""
    kind = cfg.block_kind(k)
    return kind if kind == "broadcast" else "wino_" + kind


# kind: (max err, least identical fraction).  Beside each: the twin's worst err / least identical over NETS on
# positions(), then over the GPU test's batches; then what one MI355X measured (tests/test_winograd_gpu.py).  The margins
# are trunk_emulation.BOUNDS' own: lw_btl 1.86 x / -0.067, lw_nbt 2.0 x / -0.06, classic 2.0 x / -0.074.
BLOCK_BOUNDS = {
    "wino_btl": (4.0, 0.53),       # twin 2.03 / 0.600 (test_b3c384btl3), 2.12 / 0.610; MI355X 1.95 / 0.610
    "wino_nbt": (8.5, 0.40),       # twin 4.14 / 0.464 (test_b3c384nbt), 4.27 / 0.461; MI355X 4.18 / 0.462
    "wino_classic": (7.0, 0.42),   # twin 3.26 / 0.497 (test_b3c192classic), 3.51 / 0.492 (test_b3c128classic, batch 41);
                                   # MI355X 3.49 / 0.493
}
TWIN = {"wino_btl": (2.12, 0.600), "wino_nbt": (4.27, 0.461), "wino_classic": (3.51, 0.492)}
# kind: (worst err, least identical) on one MI355X with 256 CUs (tests/test_winograd_gpu.py test_blocks_teacher_forced, the
# eight nets at batches 3, 5 and the second-unit batch 28 - 82); whole nets there: the largest raw-output error to float64
# 1.1e-3 (test_b4c512btl3_i2) to 1.8e-3 (test_b3c384nbt), 0.25 - 0.43 of WHOLE_NET's bounds
GPU_MEASURED = {"wino_btl": (1.95, 0.610), "wino_nbt": (4.18, 0.462), "wino_classic": (3.49, 0.493)}


def block_bounds():
    """trunk_emulation.BOUNDS with the Winograd kinds"""
    b = dict(te.BOUNDS)
    b.update(BLOCK_BOUNDS)
    return b


def teacher_forced(t, xs_engine, pos, slots=None, label="", bounds=None):
    """conv_widths_common.teacher_forced under the Winograd kinds: the stem and every block of WTrunk `t` checked from the
    engine's own x before it.  Returns {"stem" or block: stats}.  bounds: overrides (the measurement passes none at all)."""
    cfg = t.cfg
    C = cfg.channels
    B = block_bounds() if bounds is None else bounds
    xs = [torch.from_numpy(np.asarray(x, np.float64).reshape(len(x), C, 19, 19)) for x in xs_engine]
    x0 = t.stem(pos)
    out = {"stem": te.check_block(xs[0], x0, te.rms(x0), f"{label}stem", slots, *B["stem"])}
    for k in range(len(xs) - 1):
        m = t.block(k, xs[k])
        out[k] = te.check_block(xs[k + 1], m, te.block_scale(xs[k], m), f"{label}{k} ({kind_of(cfg, k)})", slots,
                                *B[kind_of(cfg, k)])
    return out


def outputs(cfg, W, pos):
    """conv_widths_common.outputs of the emulation"""
    import tfm_restatement
    t = WTrunk(cfg, W)
    x = t.trunk(features=pos)[-1]
    Wh = {k: (v.astype(np.float16).astype(np.float32) if k in te.HEAD_CONVS else v) for k, v in W.items()}
    out = tfm_restatement._heads(x.to(F64), Wh, x, F64)
    return {k: out[k] for k in ("raw",) + cw.PROB_KEYS}


def errors(got, ref):
    """max |d| of the raw outputs, the move probabilities and the value probabilities"""
    return {"raw": float(np.abs(np.asarray(got["raw"]) - np.asarray(ref["raw"])).max()),
            "prob": float(np.abs(np.asarray(got["move_probs"]) - np.asarray(ref["move_probs"])).max()),
            "value_prob": float(np.abs(np.asarray(got["value_probs"]) - np.asarray(ref["value_probs"])).max())}


def emulation_errors(name):
    """the emulation's own error against the float64 outputs on conv_widths_common.positions(): what WHOLE_NET is made of"""
    cfg, W = config(name), weights(name)
    pos = cw.positions()
    return errors(outputs(cfg, W, pos), cw.outputs(cfg, W, pos, fp16=False))


# The emulation's own error to float64 on conv_widths_common.positions() (python tests/winograd_restatement.py): max |d|
# of the raw outputs, the move probabilities and the value probabilities.  FP16_EMULATED: the fp16 plan's emulation
# (conv_widths_common.outputs(..., fp16=True)) on the same positions, for comparison: the two plans are about as far
# from float64 on these nets.
EMULATED = {
    "test_b3c64btl2": (1.12e-3, 1.81e-6, 1.72e-4),
    "test_b3c192btl3": (1.03e-3, 2.21e-6, 8.21e-5),
    "test_b3c96nbt": (1.74e-3, 3.62e-6, 1.24e-4),
    "test_b3c384btl3": (9.38e-4, 3.54e-6, 6.09e-5),
    "test_b3c384nbt": (1.42e-3, 3.00e-6, 1.48e-4),
    "test_b3c192classic": (1.09e-3, 2.80e-6, 4.49e-5),
    "test_b3c128classic": (1.41e-3, 3.46e-6, 1.72e-4),
    "test_b4c512btl3_i2": (1.45e-3, 3.61e-6, 6.81e-5),
}
FP16_EMULATED = {
    "test_b3c64btl2": (1.23e-3, 2.09e-6, 1.91e-4),
    "test_b3c192btl3": (9.24e-4, 2.52e-6, 6.44e-5),
    "test_b3c96nbt": (1.51e-3, 4.43e-6, 1.43e-4),
    "test_b3c384btl3": (9.78e-4, 2.26e-6, 1.23e-4),
    "test_b3c384nbt": (1.51e-3, 2.98e-6, 1.56e-4),
    "test_b3c192classic": (1.01e-3, 2.51e-6, 3.41e-5),
    "test_b3c128classic": (1.05e-3, 3.39e-6, 1.06e-4),
    "test_b4c512btl3_i2": (1.30e-3, 3.17e-6, 7.65e-5),
}
# three times EMULATED, rounded up at the second digit (int8_conv3_restatement.BOUNDS' rule)
WHOLE_NET = {
    "test_b3c64btl2": {"raw": 3.4e-3, "prob": 5.5e-6, "value_prob": 5.2e-4},
    "test_b3c192btl3": {"raw": 3.2e-3, "prob": 6.7e-6, "value_prob": 2.5e-4},
    "test_b3c96nbt": {"raw": 5.3e-3, "prob": 1.1e-5, "value_prob": 3.8e-4},
    "test_b3c384btl3": {"raw": 2.9e-3, "prob": 1.1e-5, "value_prob": 1.9e-4},
    "test_b3c384nbt": {"raw": 4.3e-3, "prob": 9.1e-6, "value_prob": 4.5e-4},
    "test_b3c192classic": {"raw": 3.3e-3, "prob": 8.5e-6, "value_prob": 1.4e-4},
    "test_b3c128classic": {"raw": 4.3e-3, "prob": 1.1e-5, "value_prob": 5.2e-4},
    "test_b4c512btl3_i2": {"raw": 4.4e-3, "prob": 1.1e-5, "value_prob": 2.1e-4},
}


def second_unit_batch(cfg, n_cu, grid_of):
    """The first batch at which a workgroup of k_wconv takes a second unit of work on a device of n_cu CUs; grid_of(npos,
    cout) -> (grid, units) is the engine's grid hook (p3achygo_amd.engine.debug_wconv_grid)."""
    cout = cw.padded(conv3_width(cfg))
    n = 1
    while True:
        grid, units = grid_of(n, cout)
        if units > grid:
            return n
        n += 1


def twin_stats(name, pos, slots=None, bounds=None):
    """{kind: (worst err, least identical)} of the twin chained through the net, every block checked from the twin's own x"""
    cfg, W = config(name), weights(name)
    xt = WTrunk(cfg, W, twin=True).trunk(pos)
    st = teacher_forced(WTrunk(cfg, W), xt, pos, slots=slots, label=f"{name} block ", bounds=bounds)
    fam = {}
    for k, v in st.items():
        f = "stem" if k == "stem" else kind_of(cfg, k)
        a = fam.setdefault(f, [0.0, 1.0])
        a[0], a[1] = max(a[0], v["max_err"]), min(a[1], v["identical"])
    return fam


def gpu_batches(cfg, n_cu=256):
    """the batches of tests/test_winograd_gpu.py's block test on a device of n_cu CUs, from the cut's own rule
    (conv_wino.h: units = ceil(100 npos / 32) * cout / 64, grid = min(units, n_cu))"""
    def grid_of(npos, cout):
        units = -(-100 * npos // 32) * (cout // 64)
        return min(units, n_cu), units
    return (3, 5, second_unit_batch(cfg, n_cu, grid_of))


if __name__ == "__main__":   # the measurements behind TWIN, BLOCK_BOUNDS, EMULATED and WHOLE_NET
    from test_conv_widths_gpu import block_batch
    names = sys.argv[1:] or NETS
    UNBOUNDED = {k: (float("inf"), 0.0) for k in block_bounds()}
    total, total_gpu = {}, {}
    for n in names:
        cfg = config(n)
        fam = twin_stats(n, cw.positions(), bounds=UNBOUNDED)
        print(n, "twin on positions():", {k: (round(a, 2), round(b, 3)) for k, (a, b) in fam.items()}, flush=True)
        for k, (a, b) in fam.items():
            t = total.setdefault(k, [0.0, 1.0])
            t[0], t[1] = max(t[0], a), min(t[1], b)
        for batch in gpu_batches(cfg):
            pos, slots = block_batch(batch)
            fam = twin_stats(n, pos[slots], slots, bounds=UNBOUNDED)
            print(n, "twin at batch", batch, {k: (round(a, 2), round(b, 3)) for k, (a, b) in fam.items()}, flush=True)
            for k, (a, b) in fam.items():
                t = total_gpu.setdefault(k, [0.0, 1.0])
                t[0], t[1] = max(t[0], a), min(t[1], b)
        W, pos = weights(n), cw.positions()
        ref = cw.outputs(cfg, W, pos, fp16=False)
        e, e16 = errors(outputs(cfg, W, pos), ref), errors(cw.outputs(cfg, W, pos, fp16=True), ref)
        print(n, "emulation to float64:", {k: float(f"{v:.3g}") for k, v in e.items()},
              "fp16 emulation:", {k: float(f"{v:.3g}") for k, v in e16.items()}, flush=True)
    print("twin, NETS:", {k: (round(a, 2), round(b, 3)) for k, (a, b) in total.items()})
    print("twin, GPU batches:", {k: (round(a, 2), round(b, 3)) for k, (a, b) in total_gpu.items()})
