"""The low-latency plan (P3HIP_FLAG_LOW_LATENCY: k_sconv of csrc/conv_split.hip, a position split across workgroups) on
the HIP engine, through the C ABI: parity with the float64 restatement at small batches, every split of the kernel's sets
bit for bit, every block on its own against the fp16 emulation, the stem and the zero padding, more items than the grid
and fewer, compaction, RUN_ALL_SLOTS, launch-graph replay, the NN cache, symmetry averaging and AUX, activation offsets
past 2^31 elements, the timing hook and an evaluation match with one low-latency player.

Tolerances (tests/low_latency_common.py): the plan has the rounding points of the runtime-width layer-wise plan, so the
nets of netspec.WIDE_CONV_CONFIGS take the table of tests/test_conv_widths_gpu.py, and the four nets whose default plan
is the fused block kernel the table tests/test_low_latency_cpu.py measures; all through conv_widths_common.tolerance.
Block by block: trunk_emulation.BOUNDS "stem", "lw_btl", "lw_nbt", "classic" and "broadcast".
"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_widths_common as cw  # noqa: E402
import low_latency_common as ll  # noqa: E402
from conftest import ROOT  # noqa: E402
from test_conv_widths_gpu import block_batch  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = ll.tolerances()
COMPOSE_NET = "test_b3c192btl3"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> .p3w of netspec.generate_weights(cfg, randomize=True), written on demand"""
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("low_latency")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = os.path.join(d, name + ".p3w")
            netspec.save_p3w(cache[name], ll.config(name), ll.weights(name))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def reference():
    """name -> (positions, float64 outputs of them), computed once per net"""
    cache = {}

    def get(name):
        if name not in cache:
            pos = cw.positions()
            cache[name] = (pos, cw.outputs(ll.config(name), ll.weights(name), pos, fp16=False))
        return cache[name]
    return get


@pytest.fixture(autouse=True)
def _no_override(monkeypatch):
    monkeypatch.delenv("P3HIP_SPLIT", raising=False)
    monkeypatch.delenv("P3HIP_DEBUG_STOP_BLOCK", raising=False)


def _engine(path, batch, extra=0):
    from p3achygo_amd import engine
    return engine.HipEngine(path, batch, flags=engine.FLAG_LOW_LATENCY | extra)


def _raws(eng, slots):
    return [eng.get_raw(s).copy() for s in slots]


@pytest.mark.parametrize("name", ll.WIDE_NETS + ll.FUSED_NETS)
def test_engine_matches_the_restatement_at_small_batches(built, files, reference, name):
    """batch 1, 3, 8 and 37; slot s holds reference position (7 s + batch) mod 16; slots holding the same position are
    bit-identical across slots and batch sizes (each batch size takes another split: the chooser's)"""
    pos, ref = reference(name)
    n = len(pos)
    seen = {}
    for batch in (1, 3, 8, 37):
        idx = (7 * np.arange(batch) + batch) % n
        eng = _engine(files(name), batch)
        eng.load_all(pos[idx])
        eng.RunInference()
        raws = np.stack(_raws(eng, range(batch)))
        for s in range(batch):
            i = int(idx[s])
            if i not in seen:
                seen[i] = raws[s].copy()
            assert np.array_equal(raws[s], seen[i]), (name, batch, s)
            cw.check_outputs(name, TOL[name], raws[s], eng.GetBatch(s), ref, i)
            own = eng.GetOwnership(s)
            assert np.abs(own - ref["raw"][i][1526:1887]).max() <= TOL[name]["logit"]
            assert np.array_equal(own, raws[s][1526:1887])
        eng.close()


_CHILD = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np
from p3achygo_amd import engine, features
out = {}
pos = features.random_positions(5, seed=43)
for split in sys.argv[2].split(";"):
    os.environ["P3HIP_SPLIT"] = split            # read at p3hip_create
    for spec in sys.argv[3:]:
        name, path = spec.split("=", 1)
        eng = engine.HipEngine(path, 5, flags=engine.FLAG_LOW_LATENCY)
        eng.load_all(pos)
        eng.RunInference()
        out["%%s:%%s" %% (name, split)] = np.stack([eng.get_raw(s) for s in range(5)])
        eng.close()
np.savez(sys.argv[1], **out)
"""


def test_every_split_gives_the_same_bits(built, files, tmp_path):
    """every (S, T) of the kernel's sets forced with P3HIP_SPLIT (a child process, so that this one's environment stays
    as it is): the raw outputs at batch 5 equal those of P3HIP_SPLIT=1,64 byte for byte.  test_b3c96nbt has padded C and
    C_b, test_b5c256btl2_i2 broadcast blocks at every second block; S = 2 and S = 4 have unequal strips"""
    names = ["test_b3c96nbt", "test_b5c256btl2_i2"]
    splits = ["%d,%d" % st for st in ll.SPLITS]
    assert "1,64" in splits and len(splits) == 9
    outp = tmp_path / "splits.npz"
    env = dict(os.environ)
    env.pop("P3HIP_SPLIT", None)
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, str(outp), ";".join(splits)] +
                       ["%s=%s" % (n, files(n)) for n in names], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(outp)
    for name in names:
        want = got["%s:1,64" % name]
        assert np.abs(want).max() > 0 and not np.isnan(want).any()
        for split in splits:
            a = got["%s:%s" % (name, split)]
            assert a.tobytes() == want.tobytes(), (name, split, np.argwhere(a != want)[:5])


def _engine_xs(path, cfg, pos, slots, flags):
    """x after the stem and after every block (P3HIP_DEBUG_STOP_BLOCK, read at create), cut to the file's C"""
    from p3achygo_amd import engine
    C, Cp = cfg.channels, cw.padded(cfg.channels)
    xs = []
    try:
        for stop in range(cfg.blocks + 1):
            os.environ["P3HIP_DEBUG_STOP_BLOCK"] = str(stop)
            eng = engine.HipEngine(path, len(pos), flags=flags)
            eng.load_all(pos)
            eng.RunInference()
            xs.append(eng.debug_x(len(pos), Cp)[slots][:, :C])
            eng.close()
    finally:
        os.environ.pop("P3HIP_DEBUG_STOP_BLOCK", None)
    return xs


@pytest.mark.parametrize("name", ll.BLOCK_NETS)
def test_blocks_teacher_forced(built, files, name):
    """the stem and every block from the engine's own x before it, inside trunk_emulation's layer-wise bounds"""
    from p3achygo_amd import engine
    cfg, W = ll.config(name), ll.weights(name)
    for batch in (1, 37):
        pos, slots = block_batch(batch)
        xs = _engine_xs(files(name), cfg, pos, slots, engine.FLAG_LOW_LATENCY)
        st = cw.teacher_forced(cw.trunk(cfg, W), xs, pos[slots], slots=slots, label=f"{name} batch {batch} block ",
                               bounds=ll.BLOCK_BOUNDS[name])
        print(name, batch, {k: (round(v["max_err"], 2), round(v["identical"], 3)) for k, v in st.items()})


def test_stem_is_the_runtime_width_plans_bit_for_bit(built, files):
    """P3HIP_DEBUG_STOP_BLOCK=0: x after the stem equals a plain (ConvAny) engine's, the same kernel"""
    from p3achygo_amd import engine
    cfg = ll.config(COMPOSE_NET)
    pos, _ = block_batch(9)
    assert engine.debug_plan(files(COMPOSE_NET), 0)[0] == "ConvAny"
    xs = []
    os.environ["P3HIP_DEBUG_STOP_BLOCK"] = "0"
    try:
        for flags in (engine.FLAG_LOW_LATENCY, 0):
            eng = engine.HipEngine(files(COMPOSE_NET), len(pos), flags=flags)
            eng.load_all(pos)
            eng.RunInference()
            xs.append(eng.debug_x(len(pos), cw.padded(cfg.channels)))
            eng.close()
    finally:
        os.environ.pop("P3HIP_DEBUG_STOP_BLOCK", None)
    assert np.abs(xs[0]).max() > 0 and xs[0].tobytes() == xs[1].tobytes()


def test_padded_channels_of_the_stream_are_exactly_zero(built, files, reference):
    name = "test_b3c96nbt"
    C = ll.config(name).channels
    pos, _ = reference(name)
    eng = _engine(files(name), len(pos))
    eng.load_all(pos)
    eng.RunInference()
    x = eng.debug_x(len(pos), cw.padded(C))
    eng.close()
    assert np.all(x[:, C:] == 0)
    assert (np.abs(x[:, :C]).max(axis=(0, 2)) > 0).all()


def test_more_items_than_the_grid(built, files, reference):
    """batch 300 on test_b3c64btl2: 300 (position, 64 channels, whole board) items on fewer workgroups, so the item loop
    wraps; every slot bit-identical to a 16-position run"""
    from p3achygo_amd import engine
    name = "test_b3c64btl2"
    assert engine.debug_split(300, 3, 64) == (1, 64) and engine.debug_split(300, 1, 64) == (1, 64)
    pos, ref = reference(name)
    small = _engine(files(name), 16)
    small.load_all(pos)
    small.RunInference()
    want = _raws(small, range(16))
    small.close()
    idx = (7 * np.arange(300) + 300) % 16
    eng = _engine(files(name), 300)
    eng.load_all(pos[idx])
    eng.RunInference()
    for s in range(300):
        assert np.array_equal(eng.get_raw(s), want[idx[s]]), s
    for s in (0, 150, 299):
        cw.check_outputs(name, TOL[name], eng.get_raw(s), eng.GetBatch(s), ref, int(idx[s]))
    eng.close()


def test_one_position_takes_the_finest_split(built, files, reference):
    """batch 1 on test_b4c512btl3_i2: the chooser's finest split on the C_b = 128 convs, 4 strips of 16-channel tiles"""
    from p3achygo_amd import engine
    name = "test_b4c512btl3_i2"
    assert engine.debug_split(1, 3, 128) == (4, 16) and engine.debug_split(1, 1, 512) == (4, 16)
    assert engine.debug_split(37, 3, 128) != (4, 16)
    pos, ref = reference(name)
    eng = _engine(files(name), 1)
    eng.load_all(pos[3:4])
    eng.RunInference()
    cw.check_outputs(name, TOL[name], eng.get_raw(0), eng.GetBatch(0), ref, 3)
    eng.close()


def test_compaction_and_run_all_slots(built, files, reference):
    from p3achygo_amd import engine
    name = COMPOSE_NET
    pos, ref = reference(name)
    eng = _engine(files(name), 40)
    for s in range(32):
        eng.LoadBatch(s, pos[s % 16:s % 16 + 1])
    eng.RunInference()
    full = _raws(eng, range(32))
    part = [2, 9, 10, 31]
    for s in part:
        eng.LoadBatch(s, pos[s % 16:s % 16 + 1])
    eng.RunInference()
    assert all(np.array_equal(a, full[s]) for a, s in zip(_raws(eng, part), part))
    eng.close()
    eng = _engine(files(name), 8, engine.FLAG_RUN_ALL_SLOTS)
    eng.LoadBatch(5, pos[5:6])
    eng.RunInference()
    assert np.array_equal(eng.get_raw(5), full[5])
    cw.check_outputs(name, TOL[name], eng.get_raw(5), eng.GetBatch(5), ref, 5)
    eng.GetBatch(0)                                      # every slot of the static batch was run
    eng.close()


def test_launch_graph_replays_bit_for_bit(built, files, reference):
    from p3achygo_amd import engine
    pos, _ = reference(COMPOSE_NET)
    B = 12
    tiled = pos[np.arange(B) % 16]
    ref = _engine(files(COMPOSE_NET), B)
    gr = _engine(files(COMPOSE_NET), B, engine.FLAG_LAUNCH_GRAPH)
    ref.load_all(tiled)
    ref.RunInference()
    want = _raws(ref, range(B))
    for rnd in range(4):                       # eager, capture, replay, replay
        gr.load_all(tiled)
        gr.RunInference()
        assert all(np.array_equal(a, b) for a, b in zip(want, _raws(gr, range(B)))), rnd
        assert gr.graph_state() == (1 if rnd >= 1 else 0)
    ref.close()
    gr.close()


def test_nn_cache_hits_are_bit_identical(built, files, reference):
    pos, _ = reference(COMPOSE_NET)
    key = lambda i: (0x9E3779B97F4A7C15 * (i + 1) & (2**64 - 1), 0xC2B2AE3D27D4EB4F * (i + 7) & (2**64 - 1))
    eng = _engine(files(COMPOSE_NET), 16)
    eng.EnableCache(8)
    for s in range(16):
        eng.LoadBatchKeyed(s, pos[s:s + 1], *key(s), symmetry=s % 8)
    eng.RunInference()
    want = _raws(eng, range(16))
    for s in range(16):
        k = 15 - s
        eng.LoadBatchKeyed(s, pos[(k + 5) % 16:(k + 5) % 16 + 1], *key(k), symmetry=1)
    eng.RunInference()
    for s in range(16):
        _, sym, hit = eng.GetBatchKeyed(s)
        assert hit and sym == (15 - s) % 8 and np.array_equal(eng.get_raw(s), want[15 - s])
    eng.close()


def test_symmetry_averaging_is_the_restated_reduce(built, files):
    """the k-copy reduce of tests/symavg_restatement.py over a low-latency engine's copies, bit for bit (the copies run
    at 8 n positions, the averaging engine's passes at k n: other splits, the same bits)"""
    from p3achygo_amd import engine, features
    from test_symmetry_avg_gpu import _check_rule
    _check_rule(files(COMPOSE_NET), features.random_positions(5, seed=47), engine.symmetry_maps()[0], masks=(0x01, 0x81, 0xFF),
                flags=engine.FLAG_LOW_LATENCY)


def test_aux_on_top_keeps_every_other_outputs_bits(built, files, reference):
    from p3achygo_amd import engine
    pos, _ = reference(COMPOSE_NET)

    def run(eng):
        eng.load_all(pos)
        eng.RunInference()
        out = []
        for s in range(16):
            r = eng.GetBatch(s)
            out.append(np.concatenate([eng.get_raw(s), np.ctypeslib.as_array(r.move_probs), np.ctypeslib.as_array(r.value_probs),
                                       np.ctypeslib.as_array(r.score_probs), eng.GetOwnership(s)]).astype(np.float32))
        return np.stack(out)
    plain = _engine(files(COMPOSE_NET), 16)
    want = run(plain)
    plain.close()
    aux = _engine(files(COMPOSE_NET), 16, engine.FLAG_AUX)
    got = run(aux)
    recs = np.stack([aux.GetAux(s) for s in range(16)])
    aux.close()
    assert want.tobytes() == got.tobytes()
    assert np.isfinite(recs).all() and np.abs(recs).max() > 0


def test_activation_offsets_past_2_31_elements_c512(built, files):
    """12,288 rows of 512 x 361 activations: the element offset of a row passes 2^31 from row index 11,619 on; every
    slot bit-identical to a 61-position run of the same position (the shape of
    tests/test_conv_widths_gpu.py test_activation_offsets_past_2_31_elements_c512)"""
    from p3achygo_amd import features
    name, npos, rows = "test_b3c512nbt", 61, 12288
    assert rows * 512 * 361 > 11619 * 512 * 361 > 2 ** 31 > 11618 * 512 * 361
    pos = features.random_positions(npos, seed=61, n_games=41, max_moves=330, komis=(7.5, -7.5, 0.5))

    def out(eng, s):
        r = eng.GetBatch(s)
        return np.concatenate([eng.get_raw(s), np.ctypeslib.as_array(r.move_probs),
                               np.ctypeslib.as_array(r.value_probs)]).astype(np.float32).view(np.uint32)
    eng = _engine(files(name), npos)
    eng.load_all(pos)
    eng.RunInference()
    ref = [out(eng, s) for s in range(npos)]
    eng.close()
    eng = _engine(files(name), rows)
    idx = (7 * np.arange(rows) + rows) % npos
    eng.load_all(pos[idx])
    eng.RunInference()
    bad = [s for s in range(rows) if not np.array_equal(out(eng, s), ref[idx[s]])]
    eng.close()
    assert not bad, (len(bad), bad[:8], [b for b in bad if b >= 11619][:8])


@pytest.mark.parametrize("name", ["test_b3c96nbt", "test_b3c128classic", "test_b3c256btl1"])
def test_trunk_kernel_timing_names_the_split_conv(built, files, reference, name):
    pos, _ = reference(name)
    cfg = ll.config(name)
    w3 = cfg.channels if cfg.block_type == "classic" else cfg.bottleneck_channels   # the file's width, unpadded
    eng = _engine(files(name), 8)
    eng.load_all(pos[:8])
    eng.upload()
    ms, fl, kname = eng.time_trunk_kernel(8, 2)
    eng.close()
    assert ms > 0 and kname == "k_sconv<3>" and fl == 2.0 * 9 * w3 * w3 * 361 * 8


def test_eval_match_with_one_low_latency_player(built, files):
    from p3achygo_amd import host_api
    w = files("test_b3c256btl1")
    try:
        host_api.eval_set_player_flags(cur="n: 16\n", cand="n: 16\nnn_low_latency: 1\n")
        st = host_api.eval_match(w, w, num_games=2, visits_per_move=16, leaves_per_round=4, max_moves=24, num_threads=2, seed=2)
    finally:
        host_api.eval_set_player_flags()
    assert st.games == 2 and st.cur_wins + st.cand_wins + st.draws == 2
