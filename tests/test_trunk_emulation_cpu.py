"""CPU checks of tests/trunk_emulation.py: the float64 mode against the goldens, the fp16 storage scheme against the
GPU bounds of test_engine_gpu.py, the twin against the block checker's thresholds, and the checker's power: each slip
M1 - M6 injected into the twin must fail it, naming the block and, where one applies, the region or channel group."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import trunk_emulation as te  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_engine_gpu import LOGIT_TOL, NETS, PEAK_PROB_TOL, PROB_TOL, VALUE_PROB_TOL, _logits_close  # noqa: E402

from p3achygo_amd import netspec  # noqa: E402

torch.set_num_threads(min(16, os.cpu_count() or 1))


def _fixture(name):
    g, pos = load_golden(name)
    cfg = netspec.CONFIGS[name[:-len("_peaked")] if name.endswith("_peaked") else name]
    W = netspec.generate_weights(cfg, randomize=True)
    if float(g["peak"]):
        W = netspec.peak_policy(W, float(g["peak"]))
    return cfg, W, g, pos


def _softmax(z):
    z = z - z.max(-1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(-1, keepdims=True)


@pytest.mark.parametrize("name", NETS)
def test_float64_mode_reproduces_goldens(name):
    cfg, W, g, pos = _fixture(name)
    planes, sc = te.inputs(pos)
    assert np.array_equal(planes, g["planes"].astype(np.float32)) and np.array_equal(sc, g["scalars"])
    raw = te.Trunk(cfg, W, fp16=False).forward(pos)
    ref = g["raw"].astype(np.float64)
    # the full-size fixtures store float32: equal to within that storage's rounding
    tol = 1e-9 + (2.0 ** -24 * np.abs(ref) if g["raw"].dtype == np.float32 else 0.0)
    assert (np.abs(raw - ref) <= tol).all(), np.abs(raw - ref).max()


# Share of LOGIT_TOL that fp16 storage alone uses per fixture: max |d| of the emulation's raw outputs against the
# float64 golden over LOGIT_TOL (x12 for the peaked policy logits).  The record of DESIGN.md section 2; the test holds
# the emulation to it within STORAGE_SHARE_SLACK, so the record cannot drift from the code.
STORAGE_SHARE = {
    "test_b3c128btl2": 0.123, "test_b3c128nbt": 0.145, "test_b3c256btl1": 0.157, "test_b3c256nbt": 0.226,
    "test_b3c384btl3": 0.132, "test_b3c384nbt": 0.150, "test_b3c192classic": 0.146, "test_b5c256nbt_i2": 0.272,
    "test_b5c128btl1_i2": 0.303, "test_b5c256btl2_i2": 0.109, "test_b10c256btl1_i2": 0.445, "b8c128nbt": 0.856,
    "b12c128btl3": 0.414, "b12c256btl3": 0.756, "b12c256btl3_peaked": 0.421, "b10c384nbt": 0.890, "b14c384btl3": 0.431,
}
STORAGE_SHARE_SLACK = 0.005


@pytest.mark.parametrize("name", NETS)
def test_fp16_storage_alone_stays_inside_the_engine_bounds(name):
    """The error the fp16 storage points alone produce, against the float64 goldens: under the bounds the GPU tests
    hold the engine to (test_engine_gpu.py _check), and as recorded in STORAGE_SHARE."""
    cfg, W, g, pos = _fixture(name)
    raw = te.Trunk(cfg, W, fp16=True).forward(pos)
    ref = g["raw"].astype(np.float64)
    peak = float(g["peak"])
    pol = peak if peak else 1.0
    share = max(np.abs(raw[:, :724] - ref[:, :724]).max() / (LOGIT_TOL * pol), np.abs(raw[:, 724:] - ref[:, 724:]).max() / LOGIT_TOL)
    print(f"{name}: storage error {share:.3f} of LOGIT_TOL")
    assert abs(share - STORAGE_SHARE[name]) <= STORAGE_SHARE_SLACK, (name, share)
    for i in range(len(pos)):
        assert _logits_close(raw[i, :724], ref[i, :724], pol)
        assert _logits_close(raw[i, 724:1887], ref[i, 724:1887])
        assert np.abs(raw[i, 1887:] - ref[i, 1887:]).max() <= LOGIT_TOL
    for lo, hi, key, tol in ((0, 362, "move_probs", PEAK_PROB_TOL if peak else PROB_TOL),
                             (362, 724, "opt_move_probs", PEAK_PROB_TOL if peak else PROB_TOL),
                             (724, 726, "value_probs", VALUE_PROB_TOL), (726, 1526, "score_probs", PROB_TOL)):
        assert np.abs(_softmax(raw[:, lo:hi]) - g[key]).max() <= tol, key


@pytest.mark.parametrize("name", NETS)
def test_twin_passes_the_block_checker(name):
    """The twin (engine storage points, other fp32 arithmetic) chained through the trunk, every block checked from the
    twin's own x before it, as the GPU test checks the engine: inside every bound."""
    cfg, W, g, pos = _fixture(name)
    xt = te.Trunk(cfg, W, twin=True).trunk(pos)
    st = te.teacher_forced(te.Trunk(cfg, W), xt, pos)
    print(name, {(k if k == "stem" else f"{k} {te.kind_of(cfg, k)}"): (round(v["max_err"], 2), round(v["identical"], 3))
                 for k, v in st.items()})


def test_twin_on_the_gpu_test_batches():
    """The twin in place of the engine on every job of test_trunk_blocks_gpu.py (its batches, sampled slots and
    hand-made positions, the hot nets among them): inside every bound, and the hot nets inside fp16."""
    import test_trunk_blocks_gpu as G
    fam: dict = {}
    for name, batch in G.BLOCK_JOBS:
        if name.endswith(":m1"):
            continue
        cfg, W, _ = G._weights(name)
        pos, slots, _ = G._batch(name, batch)
        hot = name.endswith(":hot")
        xt = te.Trunk(cfg, W, twin=True).trunk(pos[slots])
        if hot:
            top = max(float(x.abs().max()) for x in te.Trunk(cfg, W).trunk(pos[slots]))
            assert 100 < top < 4096, (name, top)
        st = te.teacher_forced(te.Trunk(cfg, W), xt, pos[slots], slots=slots, label=f"{name} block ", hot=hot)
        for k, v in st.items():
            f = "stem" if k == "stem" else ("hot" if hot else te.kind_of(cfg, k))
            a = fam.setdefault(f, [1.0, 0.0])
            a[0], a[1] = min(a[0], v["identical"]), max(a[1], v["max_err"])
    print({f: (round(b, 2), round(a, 3)) for f, (a, b) in sorted(fam.items())})


def test_heads_twin_far_below_logit_tol():
    """heads() in float32 against float64 on the same trunk output: the bound test_trunk_blocks_gpu.py holds k_headsx
    and k_heads to (HEADS_TOL) is ten times the worst of the fixtures here (1.5e-5, b12c256btl3_peaked)."""
    worst = 0.0
    for name in ("test_b3c256btl1", "test_b3c384nbt", "b12c256btl3_peaked", "b8c128nbt"):
        cfg, W, g, pos = _fixture(name)
        x = te.Trunk(cfg, W).trunk(pos)[-1]
        worst = max(worst, np.abs(te.Trunk(cfg, W, twin=True).heads(x) - te.Trunk(cfg, W).heads(x)).max())
    assert worst * 10 <= te.HEADS_TOL <= LOGIT_TOL / 10, worst


def test_engine_mish_tail():
    """The engine's mish formulas in fp32: exact 0 below y = -16.7, within MISH_TAIL_ABS of mish for every y < 0, and
    within 2e-5 relatively above y = -4; the relative error grows below (measured 3e-4 at y = -8, module docstring)."""
    y = torch.linspace(-60, 40, 200001, dtype=torch.float64)
    exact = y * torch.tanh(torch.nn.functional.softplus(y))
    for form in (True, False):
        m = te.mish_engine(y.float(), form).double()
        err = (m - exact).abs()
        assert torch.isfinite(m).all()
        assert err[y < 0].max() <= te.MISH_TAIL_ABS, float(err[y < 0].max())
        assert float((err / exact.abs().clamp_min(1e-30))[(y > -4) & (y.abs() > 1e-3)].max()) < 2e-5
    assert (te.mish_engine(y[y < -16.7].float(), True) == 0).all()
    assert float(err[y < -8].max()) > 1e-7   # the tail does lose accuracy: the floor is needed


MUTATIONS = [
    # (fixture, mutation, the block the checker must name, words its message must contain).  A slip inside a block
    # spreads to every channel through the convs after it, so the channel group and the region are named where the
    # mutated conv is the block's last: the classic block's second 3x3, the btl1 block's 3x3 before a 1x1 expand.
    ("test_b3c256btl1", dict(kind="M1", block=0, conv=1, channel=37), "block 0", []),
    ("test_b3c384nbt", dict(kind="M1", block=1, conv=2, channel=100), "block 1", []),
    ("test_b3c192classic", dict(kind="M1", block=1, conv=1, channel=37), "block 1", ["groups [4] "]),
    ("test_b3c256btl1", dict(kind="M2", block=1, conv=1), "block 1", ["regions ['corner', 'edge']"]),
    ("test_b3c192classic", dict(kind="M2", block=0, conv=1), "block 0", ["regions ['corner', 'edge']"]),
    ("test_b3c384nbt", dict(kind="M2", block=0, conv=3), "block 0", []),
    # precision slips, caught through the fraction bit-identical: M3 in the fused blocks (btl: twin 0.83 or more, M3
    # 0.60; nbt: twin 0.71 or more, M3 0.45), M4 in the C = 256 btl block (0.74).  Elsewhere they sit at the bound
    # or inside the noise of the layer-wise blocks' unrounded activations (module docstring): M3 / M4 give 0.61 / 0.64
    # in a layer-wise btl block (bound 0.62), 0.45 / 0.49 in a layer-wise nbt block (0.45), M4 0.78 in a C = 128 btl
    # block (0.78)
    ("test_b3c256btl1", dict(kind="M3", block=1), "block 1", ["identical"]),
    ("test_b3c256nbt", dict(kind="M3", block=0), "block 0", ["identical"]),
    ("test_b3c256btl1", dict(kind="M4", block=0), "block 0", ["identical"]),
    # M5: the broadcast dense normalised over 384 padded rows (the broadcast block has no gpool; trunk_emulation.py)
    ("test_b3c256btl1", dict(kind="M5", block=2), "block 2", []),
    ("test_b3c384nbt", dict(kind="M5", block=2), "block 2", []),
    ("test_b3c256btl1", dict(kind="M6", slot=1), "block stem", ["slots [1]"]),
]


@pytest.mark.parametrize("name,mut,where,words", MUTATIONS, ids=[f"{m['kind']}-{n}" for n, m, _, _ in MUTATIONS])
def test_checker_catches_mutation(name, mut, where, words):
    cfg, W, g, pos = _fixture(name)
    xt = te.Trunk(cfg, W, twin=True, mutate=mut).trunk(pos)
    emu = te.Trunk(cfg, W)
    with pytest.raises(AssertionError) as exc:
        te.teacher_forced(emu, xt, pos)
    msg = str(exc.value)
    print(msg)
    assert msg.startswith(where) and all(w in msg for w in words), msg
    # every step before the mutated one passes: the failure is localised
    bad = "stem" if mut["kind"] == "M6" else mut["block"]
    if bad != "stem":
        x0 = emu.stem(pos)
        te.check_block(xt[0], x0, te.rms(x0), "stem", None, *te.bounds(cfg, "stem"))
        for k in range(bad):
            m = emu.block(k, xt[k])
            te.check_block(xt[k + 1], m, te.block_scale(xt[k], m), k, None, *te.bounds(cfg, k))
