"""The fp32 plan of the transformer trunks (P3HIP_FLAG_FP32_TFM, csrc/transformer_f32.hip) on the HIP engine, through
the C ABI: parity with the float64 restatement at several batch sizes, every kernel of every block on its own against
float64 and the fp32 twin (teacher forcing: P3HIP_DEBUG_STOP_BLOCK, p3hip_debug_x, p3hip_debug_tfm), peaked attention,
bit-for-bit independence of batch size, slot, launch graph, RUN_ALL_SLOTS and identity-only symmetry averaging, byte
offsets past 4 GiB, P3HIP_FLAG_FP32_ANY and the timing hook.

Bounds on the outputs (tests/tfm_fp32_common.py): twice the twin's worst, rounded up to one significant digit: raw 3e-5
and probabilities 2e-6.  Kernel by kernel the error is max |a - ref| / rms(ref) against the float64 stage on the
engine's own inputs, and the engine must stay within 4 x the twin's on those inputs.

Largest errors against the float64 restatement (the fixtures' 16 positions; b14d96h3_transformer: 8), the twin on the
CPU (tests/test_transformer_fp32_cpu.py re-measures it) and the engine on an MI355X over the batches 1, 7 and 61:
                            twin raw  twin prob   MI355X raw  MI355X prob
    test_b2d64h2_tfm        3.9e-6    4.3e-7      3.02e-6     2.8e-7
    test_b2d96h3_tfm        1.15e-5   6.9e-7      1.62e-5     7.0e-7
    test_b2d128h2_tfm       5.7e-6    3.7e-7      4.41e-6     3.0e-7
    test_b2d192h6_tfm       8.7e-6    5.1e-7      1.16e-5     3.3e-7
    test_b2d256h4_tfm       6.1e-6    4.8e-7      4.61e-6     4.7e-7
    test_b2d384h12_tfm      8.6e-6    6.4e-7      4.53e-6     4.4e-7
    test_b2d384h6_tfm       8.8e-6    5.0e-7      5.12e-6     3.1e-7
    b14d96h3_transformer    1.22e-5   7.0e-7      9.85e-6     6.4e-7
Kernel by kernel on an MI355X (batch 7, both blocks), engine / twin: the projections 1.6e-6 .. 2.4e-6 against 1.6e-6 ..
2.6e-6 (ratio 0.61 .. 1.23), the attention kernel 1.8e-6 .. 3.8e-6 against 2.1e-6 .. 3.7e-6 (0.59 .. 1.17), the FFN
1.2e-6 .. 2.0e-6 against 1.5e-6 .. 2.2e-6 (0.73 .. 1.00); with Wq, Wk x 4 the attention kernel 1.5e-5 .. 2.4e-5 against
1.5e-5 .. 2.8e-5 (0.82 .. 1.02).  A first version of the attention kernel that added every key block's P . V onto the
running o (one MFMA chain over all 384 keys) measured 3.4e-6 .. 5.3e-6, up to 2.10 times the twin; every block's P . V
is now summed from zero (csrc/transformer_f32.hip).  The mutant measures 2.6 against 2.0e-6 at k
of block 1.  The whole file takes 6 s.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tfm_fp32_common as tc  # noqa: E402

pytestmark = pytest.mark.gpu

M1 = dict(block=1, head=1, lanes=(6, 7))   # Wk of block 1: two adjacent output channels of head 1 exchanged


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(name, variant) -> .p3w of the fixture weights; variant "", "hot" (Wq, Wk x 4) or "m1" (the mutant)"""
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("tfm_fp32")
    cache = {}

    def get(name, variant=""):
        if (name, variant) not in cache:
            cfg, W = tc.weights(name, hot=variant == "hot")
            if variant == "m1":
                W = dict(W)
                key = f"blocks.{M1['block']}.k.w"
                D = cfg.channels // cfg.bottleneck_channels
                a, b = (M1["head"] * D + l for l in M1["lanes"])
                w = W[key].copy()
                w[:, [a, b]] = w[:, [b, a]]
                W[key] = w
            cache[(name, variant)] = os.path.join(d, f"{name}_{variant}.p3w")
            netspec.save_p3w(cache[(name, variant)], cfg, W)
        return cache[(name, variant)]
    return get


@pytest.fixture(scope="module")
def reference():
    """name -> (positions, float64 outputs of them), computed once per net"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = tc.reference(name)
        return cache[name]
    return get


def _fp32(path, batch, flags=0):
    from p3achygo_amd import engine
    return engine.HipEngine(path, batch, flags=flags | engine.FLAG_FP32_TFM)


def _run(path, pos, flags=0, rounds=1, mask=None, fp32_flag=None):
    """raw rows of every slot of one engine of batch len(pos) after `rounds` load-and-run rounds"""
    from p3achygo_amd import engine
    eng = engine.HipEngine(path, len(pos), flags=flags | (engine.FLAG_FP32_TFM if fp32_flag is None else fp32_flag))
    if mask is not None:
        eng.set_symmetries(mask)
    for _ in range(rounds):
        eng.load_all(pos)
        eng.RunInference()
    raws = np.stack([eng.get_raw(s) for s in range(len(pos))])
    eng.close()
    return raws


@pytest.mark.parametrize("name", tc.NETS)
def test_engine_matches_the_restatement_at_batch_sizes(built, files, reference, name):
    """batch 1, 7 and 61; slot s holds fixture position (7 s + batch) mod 16; every slot is checked, and slots holding
    the same position are bit-identical across slots and batch sizes"""
    pos, ref = reference(name)
    n = len(pos)
    seen = {}
    worst = [0.0, 0.0]
    for batch in (1, 7, 61):
        idx = (7 * np.arange(batch) + batch) % n
        eng = _fp32(files(name), batch)
        eng.load_all(pos[idx])
        eng.RunInference()
        for s in range(batch):
            i = int(idx[s])
            raw = eng.get_raw(s)
            e = tc.check_outputs(name, raw, eng.GetBatch(s), eng.GetOwnership(s), ref, i, tc.RAW_TOL, tc.PROB_TOL)
            worst = [max(a, b) for a, b in zip(worst, e)]
            assert np.array_equal(raw, seen.setdefault(i, raw)), (name, batch, s)
        eng.close()
    print(f"fp32 tfm outputs {name}: raw {worst[0]:.2e} prob {worst[1]:.2e}")


def test_deep_net_matches_the_restatement(built, files, reference):
    pos, ref = reference(tc.DEEP_NET)
    eng = _fp32(files(tc.DEEP_NET), len(pos))
    eng.load_all(pos)
    eng.RunInference()
    worst = [0.0, 0.0]
    for s in range(len(pos)):
        e = tc.check_outputs(tc.DEEP_NET, eng.get_raw(s), eng.GetBatch(s), eng.GetOwnership(s), ref, s, tc.DEEP_RAW_TOL,
                             tc.DEEP_PROB_TOL)
        worst = [max(a, b) for a, b in zip(worst, e)]
    eng.close()
    print(f"fp32 tfm outputs {tc.DEEP_NET}: raw {worst[0]:.2e} prob {worst[1]:.2e}")


def _engine_record(path, cfg, pos):
    """x in front of every block and after the last, and q, k, v, o of every block (P3HIP_DEBUG_STOP_BLOCK, read at
    create), in tfm_fp32_common's layouts; asserts the padding rows and channels exactly zero and everything finite"""
    d, nh = cfg.channels, cfg.bottleneck_channels
    D, Cs, n = d // nh, tc.stream_width(d), len(pos)
    rec = {"x": [], "q": [], "k": [], "v": [], "o": []}
    old = os.environ.get("P3HIP_DEBUG_STOP_BLOCK")
    try:
        for stop in range(cfg.blocks + 1):
            os.environ["P3HIP_DEBUG_STOP_BLOCK"] = str(stop)
            eng = _fp32(path, n)
            eng.load_all(pos)
            eng.RunInference()
            x = eng.debug_x(n, Cs)
            assert np.isfinite(x).all() and (x[:, d:] == 0).all(), f"channels {d}..{Cs - 1} of x in front of block {stop}"
            rec["x"].append(tc.tokens(x, d))
            if stop > 0:
                for w, t in enumerate("qkv"):
                    a = eng.debug_tfm(w, n, nh, D)
                    assert np.isfinite(a).all() and (a[:, :, tc.L:] == 0).all(), f"rows 361..383 of {t} of block {stop - 1}"
                    rec[t].append(tc.heads_first(a))
                o = eng.debug_tfm(3, n, nh, D)
                assert np.isfinite(o).all()
                rec["o"].append(torch.from_numpy(o.astype(np.float64)))
            eng.close()
    finally:
        if old is None:
            os.environ.pop("P3HIP_DEBUG_STOP_BLOCK", None)
        else:
            os.environ["P3HIP_DEBUG_STOP_BLOCK"] = old
    return rec


def _batch7(name):
    from p3achygo_amd import features
    pos, _, _ = tc.inputs(name)
    fill = features.random_positions(7, seed=43, n_games=16, max_moves=300, komis=(7.5, -7.5, 0.5))
    fill[[0, 3, 6]] = pos[[0, 5, 11]]
    return fill


def _print_rows(name, rows):
    for kernel, t, i, eng_err, twin_err in rows:
        print(f"fp32 tfm kernels {name} block {i} {kernel} {t}: engine {eng_err:.2e} twin {twin_err:.2e} "
              f"ratio {eng_err / twin_err:.2f}")


@pytest.mark.parametrize("name", tc.KERNEL_NETS)
def test_kernels_teacher_forced(built, files, name):
    """every kernel of every block from the engine's own inputs: the error against float64 within 4 x the twin's"""
    cfg, W = tc.weights(name)
    rows = tc.kernel_rows(cfg, W, _engine_record(files(name), cfg, _batch7(name)))
    _print_rows(name, rows)
    tc.check_rows(name, rows)


def test_exchanged_channels_are_rejected_at_k_of_block_1(built, files):
    """the engine gets Wk of block 1 with two adjacent channels of head 1 exchanged, the reference does not: the check
    fails at k_tfm_qkv_f32 k of block 1 and nowhere earlier"""
    name = "test_b2d96h3_tfm"
    cfg, W = tc.weights(name)
    rows = tc.kernel_rows(cfg, W, _engine_record(files(name, "m1"), cfg, _batch7(name)))
    _print_rows(name + ":m1", rows)
    with pytest.raises(AssertionError) as exc:
        tc.check_rows(name, rows)
    assert str(exc.value).startswith(f"{name} block {M1['block']} k_tfm_qkv_f32 k:"), str(exc.value)


@pytest.mark.parametrize("name", tc.HOT_NETS)
def test_attention_kernel_with_peaked_attention(built, files, name):
    """Wq, Wk x 4: a row of the softmax is carried by a few keys and the running maximum rises between key blocks"""
    import tfm_emulation as T
    cfg, W = tc.weights(name, hot=True)
    rec = _engine_record(files(name, "hot"), cfg, _batch7(name))
    q, k = (rec[t][0].permute(0, 2, 1, 3) for t in "qk")
    reg = T.attention_regime(T.Tfm(cfg, W, fp16=False), q, k)
    print(f"fp32 tfm hot {name}: " + ", ".join(f"{a} {b:.3f}" for a, b in reg.items()))
    assert reg["peak"] >= 0.7
    rows = tc.kernel_rows(cfg, W, rec, stages=("attn",))
    _print_rows(name + ":hot", rows)
    tc.check_rows(name, rows)


def test_results_do_not_depend_on_batch_slot_graph_or_identity_symmetry(built, files, reference):
    from p3achygo_amd import engine
    name = "test_b2d192h6_tfm"
    pos, _ = reference(name)
    path = files(name)
    idx = (7 * np.arange(61) + 61) % len(pos)
    want = _run(path, pos[idx])
    alone = _fp32(path, 1)
    for i in range(len(pos)):                       # every position alone, batch 1
        alone.load_all(pos[i:i + 1])
        alone.RunInference()
        raw = alone.get_raw(0)
        for s in np.flatnonzero(idx == i):
            assert np.array_equal(want[s], raw), (i, s)
    alone.close()
    seven = _run(path, pos[idx[20:27]])             # tiles of 32 tokens span positions at other places than at batch 61
    assert np.array_equal(seven, want[20:27])
    assert np.array_equal(_run(path, pos[idx], flags=engine.FLAG_LAUNCH_GRAPH, rounds=3), want)   # eager, capture, replay
    eng = _fp32(path, 61, flags=engine.FLAG_RUN_ALL_SLOTS)
    eng.LoadBatch(5, pos[idx[5]:idx[5] + 1])
    eng.RunInference()
    assert np.array_equal(eng.get_raw(5), want[5])
    eng.close()
    assert np.array_equal(_run(path, pos[idx], flags=engine.FLAG_SYMMETRY_AVG, mask=1), want)


def test_byte_offsets_past_4_gib(built, files, reference):
    """8,192 rows of d = 384: each of q, k, v is 4.8 GB, a row's byte offset passes 2^32 from row 7,282 on; the first 61
    slots of the 1024-slot symmetry-averaged run are bit-identical to a 61-slot one"""
    from p3achygo_amd import engine
    name, batch = "test_b2d384h6_tfm", 1024
    assert 7282 * 384 * 384 * 4 > 2 ** 32 > 7281 * 384 * 384 * 4 and 8 * batch > 7282
    pos, _ = reference(name)
    idx = (7 * np.arange(batch) + 61) % len(pos)
    want = _run(files(name), pos[idx[:61]], flags=engine.FLAG_SYMMETRY_AVG)
    try:
        eng = _fp32(files(name), batch, flags=engine.FLAG_SYMMETRY_AVG)
    except engine.EngineError as e:
        if "hipMalloc" in str(e):
            pytest.skip(f"not enough device memory: {e}")
        raise
    eng.load_all(pos[idx])
    eng.RunInference()
    got = np.stack([eng.get_raw(s) for s in range(batch)])
    eng.close()
    assert np.array_equal(got[:61], want)
    first = {int(i): s for s, i in reversed(list(enumerate(idx)))}
    bad = [s for s in range(batch) if not np.array_equal(got[s], got[first[int(idx[s])]])]
    assert not bad, (len(bad), bad[:8])


def test_fp32_any_takes_the_plan_of_the_trunk(built, files, reference, weight_files):
    from p3achygo_amd import engine, features
    name = "test_b2d64h2_tfm"
    pos, _ = reference(name)
    assert np.array_equal(_run(files(name), pos[:5], fp32_flag=engine.FLAG_FP32_ANY), _run(files(name), pos[:5]))
    conv = weight_files("test_b3c128btl2")
    cpos = features.random_positions(5, seed=11)
    assert np.array_equal(_run(conv, cpos, fp32_flag=engine.FLAG_FP32_ANY), _run(conv, cpos, fp32_flag=engine.FLAG_FP32))


def test_trunk_kernel_timing_names_the_fp32_attention(built, files, reference):
    name = "test_b2d96h3_tfm"
    pos, _ = reference(name)
    eng = _fp32(files(name), 32)
    eng.load_all(pos[np.arange(32) % 16])
    eng.upload()
    ms, fl, kname = eng.time_trunk_kernel(32, 2)
    assert ms > 0 and kname == "k_tfm_attn_f32" and fl == 2.0 * 32 * 2.0 * 361 * 361 * 96
    total = eng.flops_per_position()[0]
    eng.close()
    from p3achygo_amd import engine
    half = engine.HipEngine(files(name), 1)
    assert half.flops_per_position()[0] == total
    half.close()
