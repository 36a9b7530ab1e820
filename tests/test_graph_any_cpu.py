"""A captured graph for runs of every size (P3HIP_FLAG_LAUNCH_GRAPH_ANY) without a GPU: the policy of
the engine's table of graphs (csrc/graph_table.h) through p3hip_debug_graph_table, the P3HIP_GRAPH_CACHE variable, the flag
beside P3HIP_FLAG_LAUNCH_GRAPH, the hosts' switches, and the stand-alone check of the table under the address and
undefined-behaviour sanitizers (tools/graph_table_check.cpp: a program of its own, nothing is loaded into Python)."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_create_matrix_cpu import outcome

LAUNCH, CAPTURE, REPLAY = 0, 1, 2


def _golden_nets():
    """the short nets with a golden file: every trunk family and plan the engine serves"""
    from p3achygo_amd import netspec
    names = sorted(os.path.basename(p)[3:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "nn_test_*.npz")))
    return [n for n in names if n in netspec.CONFIGS]


# ---- 1. the table's policy --------------------------------------------------------------------------------------------

def test_a_key_is_launched_captured_then_replayed(built):
    from p3achygo_amd import engine
    actions, evicted = engine.debug_graph_table([8, 8, 8, 3, 3, 3, 8])
    assert actions == [0, 1, 2, 0, 1, 2, 2]
    assert evicted == [-1] * 7


def test_forward_rows_are_part_of_the_key(built):
    """8 slots as 8 rows and 8 slots as 15 rows (one slot under all eight symmetries) are two graphs"""
    from p3achygo_amd import engine
    actions, _ = engine.debug_graph_table([(8, 8), (8, 15), (8, 8), (8, 15), (8, 8), (8, 15), (7, 15)])
    assert actions == [0, 0, 1, 1, 2, 2, 0]


def test_a_full_table_gives_up_the_entry_replayed_longest_ago(built):
    from p3achygo_amd import engine
    a, b, c = 5, 6, 7
    actions, evicted = engine.debug_graph_table([a, a, b, b, c, c, a, a], capacity=2)
    assert actions == [0, 1, 0, 1, 0, 1, 0, 1]
    # c's capture (step 5) gives up a (captured at step 1), a's (step 7) gives up b (step 3): b, held, outlives the older a
    assert evicted == [-1, -1, -1, -1, -1, 1, -1, 3]
    # a replay makes an entry young again: with a replayed after b's capture, c's capture gives up b
    actions, evicted = engine.debug_graph_table([a, a, b, b, a, c, c, b], capacity=2)
    assert actions == [0, 1, 0, 1, 2, 0, 1, 0]
    assert evicted == [-1, -1, -1, -1, -1, -1, 3, -1]


def test_a_sighting_pushed_out_of_the_map_starts_again(built):
    """sightings of keys not held are counted in a map of 4 x capacity entries, the oldest forgotten first"""
    from p3achygo_amd import engine
    cap = 2
    others = list(range(100, 100 + 4 * cap))
    actions, _ = engine.debug_graph_table([9] + others + [9, 9], capacity=cap)
    assert actions == [0] * (1 + 4 * cap) + [0, 1]           # forgotten: the second sighting counts as a first
    actions, _ = engine.debug_graph_table([9] + others[:-1] + [9], capacity=cap)
    assert actions == [0] * (4 * cap) + [1]                   # one sighting fewer in between: still known


def test_capacity_one_thrashes_and_the_counts_show_it(built):
    """two keys taking turns on a table of one graph, each run twice before the other's turn (the pattern of a, a, b, b
    above): every second pass is a capture that gives up the other key's graph, and nothing is ever replayed"""
    from p3achygo_amd import engine
    keys = [4, 4, 6, 6] * 10
    actions, evicted = engine.debug_graph_table(keys, capacity=1)
    assert actions == [LAUNCH, CAPTURE] * 20
    assert actions.count(REPLAY) == 0 and actions.count(CAPTURE) == 20
    assert evicted[:2] == [-1, -1] and all(e == i - 2 for i, e in enumerate(evicted) if i >= 3 and i % 2 == 1)
    # the same keys on a table of two: two captures, the rest replays
    actions, evicted = engine.debug_graph_table(keys, capacity=2)
    assert actions.count(CAPTURE) == 2 and actions.count(REPLAY) == 36 and set(evicted) == {-1}


def test_hook_refuses_bad_capacities(built):
    from p3achygo_amd import engine
    for cap in (0, -1, 1025):
        with pytest.raises(ValueError):
            engine.debug_graph_table([1, 1], capacity=cap)
    assert engine.debug_graph_table([1, 1], capacity=1024)[0] == [0, 1]
    assert engine.debug_graph_table([])[0] == []


# ---- 2. P3HIP_GRAPH_CACHE ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", ["0", "1025", "x", "", "-3", "16k"])
def test_a_bad_graph_cache_refuses_the_engine_by_name(built, weight_files, monkeypatch, value):
    from p3achygo_amd import engine
    path = weight_files("test_b3c256btl1")
    monkeypatch.setenv("P3HIP_GRAPH_CACHE", value)
    for flags in (engine.FLAG_LAUNCH_GRAPH_ANY, engine.FLAG_LAUNCH_GRAPH_ANY | engine.FLAG_LAUNCH_GRAPH):
        with pytest.raises(engine.EngineError, match="P3HIP_GRAPH_CACHE must be a whole number of graphs from 1 to 1024"):
            engine.debug_plan(path, flags)
        with pytest.raises(engine.EngineError, match="P3HIP_GRAPH_CACHE"):
            engine.HipEngine(path, 4, flags=flags)
    # nothing else reads the variable
    assert engine.debug_plan(path, engine.FLAG_LAUNCH_GRAPH)[0] == "Fused"
    assert engine.debug_plan(path, 0)[0] == "Fused"


@pytest.mark.parametrize("value", ["1", "2", "64", "1024"])
def test_a_good_graph_cache_is_accepted(built, weight_files, monkeypatch, value):
    from p3achygo_amd import engine
    monkeypatch.setenv("P3HIP_GRAPH_CACHE", value)
    path = weight_files("test_b3c256btl1")
    assert engine.debug_plan(path, engine.FLAG_LAUNCH_GRAPH_ANY)[0] == "Fused"
    assert outcome(path, engine.FLAG_LAUNCH_GRAPH_ANY) == "accepted"


# ---- 3. the flag --------------------------------------------------------------------------------------------------------

def test_flag_value_and_exports(built):
    import re
    from p3achygo_amd import engine
    hdr = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    assert engine.FLAG_LAUNCH_GRAPH_ANY == 131072 and re.search(r"#define P3HIP_FLAG_LAUNCH_GRAPH_ANY 131072u\b", hdr)
    flags = [v for k, v in vars(engine).items() if k.startswith("FLAG_") and bin(v).count("1") == 1]
    assert len(flags) == len(set(flags))                      # the bit is nobody else's
    for name in ("p3hip_graph_stats", "p3hip_debug_graph_table"):
        assert name in engine.EXPORTS and re.search(rf"\bint {name}\(", hdr)


@pytest.mark.parametrize("name", _golden_nets())
def test_the_flag_chooses_launch_graphs_plan(built, weight_files, monkeypatch, name):
    """alone and beside FLAG_LAUNCH_GRAPH the new flag builds the plan FLAG_LAUNCH_GRAPH builds: path, quantized tensors,
    digest of the int8 weights; under the plan flags that serve the net too, and a refusal stays the same refusal"""
    from p3achygo_amd import engine
    monkeypatch.delenv("P3HIP_GRAPH_CACHE", raising=False)
    path = weight_files(name)
    G, A = engine.FLAG_LAUNCH_GRAPH, engine.FLAG_LAUNCH_GRAPH_ANY
    extras = (0, engine.FLAG_LOW_LATENCY_ANY, engine.FLAG_INT8_ANY, engine.FLAG_FP32_ANY, engine.FLAG_WINOGRAD,
              engine.FLAG_SYMMETRY_AVG, engine.FLAG_SYMMETRY_SLOT, engine.FLAG_AUX | engine.FLAG_RUN_ALL_SLOTS,
              engine.FLAG_SHARED_DEVICE)

    def plan(flags):
        try:
            return engine.debug_plan(path, flags)
        except engine.EngineError as ex:
            return str(ex)

    assert isinstance(plan(G), tuple)
    for extra in extras:
        want = plan(G | extra)
        assert plan(A | extra) == want and plan(A | G | extra) == want, hex(extra)
        assert outcome(path, A | extra) == outcome(path, G | extra) == outcome(path, A | G | extra)


def test_hosts_pass_the_flag(built, tmp_path):
    """nn_graph_any: 1 of an eval player parses, both engine-opening sites of the eval hosts pass the flag for it, and the
    self-play option passes it for the game groups' engines"""
    import ctypes as C
    from p3achygo_amd import host_api
    H = host_api.lib()
    H.p3host_parse_player_graph_any.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_char_p]
    val, err = C.c_int(-1), C.create_string_buffer(256)
    p = tmp_path / "player.cfg"
    p.write_text("n: 8\n")
    assert H.p3host_parse_player_graph_any(str(p).encode(), C.byref(val), err) == 0 and val.value == 0
    for text, want in (("nn_graph_any: 1\n", 1), ("n: 8\nnn_graph_any: 0\n", 0), ("nn_graph_any: 1\nnn_low_latency: 1\n", 1)):
        p.write_text(text)
        assert H.p3host_parse_player_graph_any(str(p).encode(), C.byref(val), err) == 0, (text, err.value)
        assert val.value == want
    for text in ("nn_graph_any: 2\n", "nn_graph_any: yes\n"):
        p.write_text(text)
        assert H.p3host_parse_player_graph_any(str(p).encode(), C.byref(val), err) == 1, text
        assert err.value.decode().startswith("nn_graph_any must be 0 or 1"), err.value
    # the match drivers' flags are written once (EvalEngineFlags) and reach both engine-opening sites through one helper
    src = open(os.path.join(ROOT, "p3achygo_amd", "host", "eval_match.cc")).read()
    assert src.count("nn_graph_any ? P3HIP_FLAG_LAUNCH_GRAPH_ANY : 0u") == 1
    assert src.count("EvalEngineFlags(c)") == 1 and src.count("= MakeEvalEvaluator(") == 2
    src = open(os.path.join(ROOT, "p3achygo_amd", "host", "selfplay.cc")).read()
    assert src.count("opt_.graph_any ? P3HIP_FLAG_LAUNCH_GRAPH_ANY : 0u") == 1
    host_api.set_graph_any(1)       # the switch exists and takes both values; off again for whoever runs next
    host_api.set_graph_any(0)


# ---- 4. the table under the sanitizers ---------------------------------------------------------------------------------

def test_table_against_a_naive_model_under_sanitizers(built, tmp_path):
    """tools/graph_table_check.cpp, built with -fsanitize=address,undefined and run as a program of its own: 10,000 random
    keys at capacities 1, 2 and 64, every step and the counters against a model that scans plain vectors"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the table's sanitizer program"
    exe = str(tmp_path / "graph_table_check")
    # the sanitizer runtimes are linked statically: the program does not care what else the loader brings in, and the
    # child runs in the environment it inherits
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tools", "graph_table_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok" and [ln.split(":")[0] for ln in lines[:3]] == ["capacity 1", "capacity 2", "capacity 64"]
    assert all("10000 steps" in ln for ln in lines[:3])
    for ln in lines[:3]:                                       # every kind of step happened at every capacity
        counts = dict(zip(ln.split(", ", 1)[1].split()[0::2], ln.split(", ", 1)[1].split()[1::2]))
        assert all(int(counts[k]) > 0 for k in ("captures", "replays", "launches", "evictions")), ln
