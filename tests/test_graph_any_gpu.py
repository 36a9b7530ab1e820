"""A captured graph for runs of every size on the MI355X (P3HIP_FLAG_LAUNCH_GRAPH_ANY).

Every test runs two engines of 8 slots with the same flags, one with the new flag and one without any graph flag, through
the same loads, and holds every output of the first against the second bit for bit: the result record, the raw row and the
ownership map of every evaluated slot, and the aux record where FLAG_AUX is set.  A replay executes the launches of the
kernel-by-kernel pass with the same arguments, so nothing may move.  What the table did is read from p3hip_graph_stats."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

B = 8
FUSED, LAYERWISE, TFM, INT8_NET = "test_b3c256btl1", "test_b3c384btl3", "test_b2d96h3_tfm", "test_b3c192classic"


@pytest.fixture(scope="module")
def nets(built, weight_files, tmp_path_factory):
    """name -> weight file: the short conv nets seeded at random, the transformer with its fixture's weights"""
    from p3achygo_amd import netspec
    from tfm_restatement import fixture_weights
    d = tmp_path_factory.mktemp("graph_any")

    def get(name):
        if name != TFM:
            return weight_files(name)
        path = str(d / "tfm.p3w")
        if not os.path.exists(path):
            cfg, W = fixture_weights(TFM)
            netspec.save_p3w(path, cfg, W)
        return path
    return get


@pytest.fixture(scope="module")
def positions(built):
    from p3achygo_amd import features
    return features.random_positions(16 * B, seed=2121, n_games=24)


def _slots(n, r):
    """n of the 8 slots, scattered, another set each run"""
    return [(3 * j + r) % B for j in range(n)]


def _outputs(eng, slots, aux=False, resident=False):
    """every output of the slots as bytes (the result record last: fetching it marks the slot)"""
    out = []
    for s in slots:
        out.append(eng.get_raw(s).tobytes())
        out.append(eng.GetOwnership(s).tobytes())
        if aux:
            out.append(eng.GetAux(s).tobytes())
        if not resident:            # (p3hip_forward_resident copies no result records back)
            out.append(bytes(eng.GetBatch(s)))
    return out


class Pair:
    """the engine under test (`gr`) and its twin without a graph flag (`ref`)"""

    def __init__(self, path, flags=0, prepare=None, **kw):
        from p3achygo_amd import engine
        self.aux = bool(flags & engine.FLAG_AUX)
        self.ref = engine.HipEngine(path, B, flags=flags, **kw)
        self.gr = engine.HipEngine(path, B, flags=flags | engine.FLAG_LAUNCH_GRAPH_ANY, **kw)
        for e in (self.ref, self.gr):
            if prepare:
                prepare(e)
        with pytest.raises(engine.EngineError):
            self.ref.graph_stats()
        self.runs = 0

    def both(self, fn):
        for e in (self.ref, self.gr):
            fn(e)

    def run(self, slots, pos, masks=None):
        """loads pos[i] into slots[i] of both engines, runs both, compares every output; returns the outputs"""
        def go(e):
            for i, s in enumerate(slots):
                e.LoadBatch(s, pos[i:i + 1])
                if masks is not None:
                    e.set_slot_symmetries(s, masks[i])
            e.RunInference()
        self.both(go)
        return self.compare(slots)

    def compare(self, slots, resident=False):
        want = _outputs(self.ref, slots, self.aux, resident)
        got = _outputs(self.gr, slots, self.aux, resident)
        assert len(got) == len(want) and all(a == b for a, b in zip(got, want)), \
            (self.runs, [i for i, (a, b) in enumerate(zip(got, want)) if a != b][:4])
        self.runs += 1
        return got

    def stats(self):
        return self.gr.graph_stats()

    def close(self):
        self.both(lambda e: e.close())


def _cases():
    from p3achygo_amd import engine
    return [(FUSED, 0), (LAYERWISE, 0), (TFM, 0), (FUSED, engine.FLAG_LOW_LATENCY), (TFM, engine.FLAG_LOW_LATENCY_TFM)]


@pytest.mark.parametrize("case", range(5))
def test_run_sizes(nets, positions, case):
    """8, 8, 8, 3, 3, 3, 5, 5, 1, 1, 1, 8 slots loaded: four keys, each launched once, captured once, and replayed from its
    third run on (5 is never run a third time)"""
    net, flags = _cases()[case]
    p = Pair(nets(net), flags)
    try:
        assert p.gr.graph_state() == 0 and p.stats() == dict(held=0, captures=0, replays=0, launched=0, evictions=0)
        for r, n in enumerate([8, 8, 8, 3, 3, 3, 5, 5, 1, 1, 1, 8]):
            p.run(_slots(n, r), positions[r * B:r * B + n])
            assert p.gr.graph_state() == (1 if r >= 1 else 0) and p.ref.graph_state() == 0
        assert p.stats() == dict(held=4, captures=4, replays=4, launched=4, evictions=0)
    finally:
        p.close()


def test_plain_launch_graph_reports_its_single_graph(nets, positions):
    from p3achygo_amd import engine
    eng = engine.HipEngine(nets(FUSED), B, flags=engine.FLAG_LAUNCH_GRAPH)
    try:
        for r, n in enumerate([8, 8, 8, 3, 3, 3]):
            for i, s in enumerate(_slots(n, r)):
                eng.LoadBatch(s, positions[i:i + 1])
            eng.RunInference()
            for s in _slots(n, r):
                eng.GetBatch(s)
        assert eng.graph_stats() == dict(held=1, captures=1, replays=1, launched=4, evictions=0)
        assert eng.graph_state() == 1
    finally:
        eng.close()


def test_nn_cache(nets, positions):
    """with the cache on a run evaluates its misses only, a partial pass over the cache's gathered copy: 5 misses out of 8
    three times replay the third time; a full run of misses and a direct full pass over the uploaded buffer read different
    buffers and hold a graph each"""
    p = Pair(nets(FUSED), prepare=lambda e: e.EnableCache(12))
    key = lambda k: ((0x9E3779B97F4A7C15 * (k + 1)) & (2**64 - 1), (0xC2B2AE3D27D4EB4F * (k + 7)) & (2**64 - 1))
    try:
        def run(slot_keys, pos):
            def go(e):
                for i, (s, k) in enumerate(slot_keys):
                    e.LoadBatchKeyed(s, pos[i:i + 1], *key(k), symmetry=0)
                e.RunInference()
            p.both(go)
            hits = [p.gr.GetBatchKeyed(s)[2] for s, _ in slot_keys]
            assert hits == [p.ref.GetBatchKeyed(s)[2] for s, _ in slot_keys]
            p.compare([s for s, _ in slot_keys])
            return hits

        hot = positions[:3]
        assert run([(s, 1000 + s) for s in range(3)], hot) == [False] * 3        # three keys into the table
        before = p.stats()
        for r in range(3):                                                        # 3 hits + 5 fresh keys, three times
            pos = np.concatenate([hot, positions[8 + 5 * r:13 + 5 * r]])
            hits = run([(s, 1000 + s) for s in range(3)] + [(s, 2000 + 10 * r + s) for s in range(3, 8)], pos)
            assert hits == [True] * 3 + [False] * 5, r
        st = p.stats()
        assert st["replays"] - before["replays"] >= 1 and st["captures"] - before["captures"] == 1
        # a full run of misses through the cache path, three times
        for r in range(3):
            assert run([(s, 3000 + 10 * r + s) for s in range(8)], positions[40 + 8 * r:48 + 8 * r]) == [False] * 8
        st2 = p.stats()
        assert st2["captures"] == st["captures"] + 1 and st2["replays"] > st["replays"]
        # and the direct full pass over the uploaded buffer, three times
        for r in range(3):
            p.both(lambda e: (e.load_all(positions[64 + 8 * r:72 + 8 * r]), e.upload(), e.forward_resident(B), e.sync()))
            p.compare(range(B), resident=True)
        st3 = p.stats()
        assert st3["captures"] == st2["captures"] + 1 and st3["replays"] == st2["replays"] + 1
        assert st3["held"] == 3 and st3["evictions"] == 0 and p.gr.graph_state() == 1
    finally:
        p.close()


def test_resident_and_run_paths_hold_a_graph_each(nets, positions):
    """p3hip_forward_resident writes no dense result records and p3hip_run does: two keys, and neither keeps the other
    from its graph"""
    p = Pair(nets(FUSED))
    try:
        for r in range(3):
            p.both(lambda e: (e.load_all(positions[8 * r:8 * r + 8]), e.upload(), e.forward_resident(B), e.sync()))
            p.compare(range(B), resident=True)
            p.run(list(range(B)), positions[32 + 8 * r:40 + 8 * r])
            want = (0, 0, 2) if r == 0 else (2, 0, 2) if r == 1 else (2, 2, 2)
            st = p.stats()
            assert (st["captures"], st["replays"], st["launched"]) == want, (r, st)
        assert p.stats()["held"] == 2 and p.gr.graph_state() == 1
    finally:
        p.close()


def test_symmetry_slot(nets, positions):
    """one slot under all eight symmetries beside seven under one: 15 forward rows, a key of its own; which slot carries
    0xFF is read from the table in device memory, so it may move between replays"""
    from p3achygo_amd import engine
    p = Pair(nets(FUSED), engine.FLAG_SYMMETRY_SLOT, symmetry_rows=24)
    try:
        def masks(root):
            return [0xFF if s == root else 1 << ((3 * s + root) % 8) for s in range(B)]
        for r, root in enumerate([2, 2, 6]):
            p.run(list(range(B)), positions[8 * r:8 * r + 8], masks(root))
        assert p.stats() == dict(held=1, captures=1, replays=1, launched=1, evictions=0)
        for r in range(3):                                    # every slot under one symmetry: 8 rows, a second key
            p.run(list(range(B)), positions[24 + 8 * r:32 + 8 * r], [1 << ((5 * s + r) % 8) for s in range(B)])
        assert p.stats() == dict(held=2, captures=2, replays=2, launched=2, evictions=0)
        p.run(list(range(B)), positions[48:56], masks(0))     # the first key again
        assert p.stats()["replays"] == 3
        # more copies than rows: refused before anything is launched, on both engines alike
        before = p.stats()
        for e in (p.ref, p.gr):
            for s in range(B):
                e.LoadBatch(s, positions[56 + s:57 + s])
                e.set_slot_symmetries(s, 0xFF if s < 4 else 0x01)
            with pytest.raises(engine.EngineError, match="symmetry_rows"):
                e.RunInference()
        assert p.stats() == before
    finally:
        p.close()


def test_symmetry_avg_mask_change_drops_the_table(nets, positions):
    from p3achygo_amd import engine
    p = Pair(nets(FUSED), engine.FLAG_SYMMETRY_AVG)
    try:
        for r in range(3):
            p.run(_slots(5, r), positions[8 * r:8 * r + 5])
        assert p.stats() == dict(held=1, captures=1, replays=1, launched=1, evictions=0)
        p.both(lambda e: e.set_symmetries(0x2D))             # four symmetries: 20 forward rows, other kernel arguments
        assert p.stats()["held"] == 0 and p.gr.graph_state() == 0
        want = [dict(held=0, captures=1, replays=1, launched=2), dict(held=1, captures=2, replays=1, launched=2),
                dict(held=1, captures=2, replays=2, launched=2)]
        for r in range(3):
            p.run(_slots(5, r), positions[24 + 8 * r:24 + 8 * r + 5])
            st = p.stats()
            assert {k: st[k] for k in want[r]} == want[r], (r, st)
        assert p.stats()["evictions"] == 0                    # a drop is no eviction
    finally:
        p.close()


def test_int8_scales_change_between_replays(nets, positions):
    """the INT8 kernels read the activation scales from device memory: new scales change a replay's results exactly as
    they change the kernel-by-kernel engine's; calibration passes never reach the table"""
    from p3achygo_amd import engine
    p = Pair(nets(INT8_NET), engine.FLAG_INT8)
    try:
        def calibrate(e):
            e.load_all(positions[:B])
            e.int8_calibrate()
            for s in range(B):      # (a slot stays in the next run until its result is fetched)
                e.GetBatch(s)
        for _ in range(3):
            p.both(calibrate)
        assert p.stats() == dict(held=0, captures=0, replays=0, launched=3, evictions=0)
        s = p.ref.int8_scales()
        assert np.array_equal(p.gr.int8_scales(), s) and (s > 0).all()
        pos = positions[8:13]
        for r in range(3):
            first = p.run(_slots(5, 0), pos)
        assert p.stats() == dict(held=1, captures=1, replays=1, launched=4, evictions=0)
        p.both(lambda e: e.set_int8_scales((s * np.float32(1.25)).astype(np.float32)))
        second = p.run(_slots(5, 0), pos)
        assert second != first and p.stats()["replays"] == 2
    finally:
        p.close()


@pytest.mark.parametrize("which", ["aux", "run_all_slots"])
def test_aux_and_run_all_slots_and_poison_between_replays(nets, positions, which):
    """FLAG_AUX: the aux record rides in the graph.  FLAG_RUN_ALL_SLOTS: every run is the full batch, one key however
    many slots were loaded.  Poisoning every scratch buffer between two replays moves no bit: the graph stays valid"""
    from p3achygo_amd import engine
    flags = engine.FLAG_AUX if which == "aux" else engine.FLAG_RUN_ALL_SLOTS
    p = Pair(nets(FUSED), flags)
    try:
        sizes = [5, 5, 5, 5] if which == "aux" else [8, 3, 5, 2]
        for r, n in enumerate(sizes):
            if r == 3:
                p.both(lambda e: e.debug_poison(0xFF))
            p.run(_slots(n, r), positions[8 * r:8 * r + n])
        assert p.stats() == dict(held=1, captures=1, replays=2, launched=1, evictions=0)
    finally:
        p.close()


def test_eviction(nets, positions, monkeypatch):
    monkeypatch.setenv("P3HIP_GRAPH_CACHE", "2")
    p = Pair(nets(FUSED))
    try:
        for r, n in enumerate([1, 2, 3, 4] * 2 + [4, 3, 1]):
            p.run(_slots(n, r), positions[8 * r:8 * r + n])
            assert p.stats()["held"] <= 2
        # second cycle: 1 and 2 captured, 3 gives up 1's graph, 4 gives up 2's; then 4 and 3 replay, 1 starts again
        assert p.stats() == dict(held=2, captures=4, replays=2, launched=5, evictions=2)
    finally:
        p.close()
