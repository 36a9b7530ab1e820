#!/usr/bin/env python3
"""Same games from two builds of libp3host.so (a refactor of the self-play scheduler against its parent).

    python tools/selfplay_split_digests.py PARENT/libp3host.so BRANCH/libp3host.so > profiles/selfplay_split_digests.txt

Each library runs in a process of its own: the "hash" evaluator, init_state_sampling off, a step limit; groups 1, 2, 3 x
(lanes, depth) (1,1), (2,1), (2,2), (2,4) x seeds 5, 12; 48 games per group, n = 16, k = 4, max_moves 24; the steps that
tests/test_selfplay_cpu.py uses for each depth, times the number of groups.  Every game runner's first-game digest is
printed.  Then the two outputs are compared: wherever both builds finished a runner's first game the digests are equal, at
least 40 of every 48 are finished in both, and with one group and one lane positions, batches, moves and games are equal.
Exit status 1 if not."""
import ctypes as C
import subprocess
import sys

GROUPS = (1, 2, 3)
LANES = ((1, 1, 560), (2, 1, 1120), (2, 2, 800), (2, 4, 700))   # lanes, depth, steps per group
SEEDS = (5, 12)
GAMES = 48


class Stats(C.Structure):
    _fields_ = [("seconds", C.c_double), ("positions", C.c_long), ("moves", C.c_long), ("games", C.c_long),
                ("black_wins", C.c_long), ("batches", C.c_long), ("gpu_seconds", C.c_double), ("host_seconds", C.c_double),
                ("cache_hits", C.c_long), ("advance_batches", C.c_long), ("games_past_opening", C.c_long),
                ("seconds_fit", C.c_double), ("rounds", C.c_long)]


def run_all(path):
    L = C.CDLL(path)
    L.p3host_selfplay_set_policy.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float]
    L.p3host_selfplay_set_step_limit.argtypes = [C.c_long]
    L.p3host_selfplay_run.argtypes = [C.c_char_p, C.c_char_p] + [C.c_int] * 8 + [C.c_double, C.c_int, C.c_uint64,
                                                                               C.POINTER(Stats), C.c_char_p]
    L.p3host_selfplay_last_first_game_digests.argtypes = [C.c_void_p, C.c_int]
    L.p3host_selfplay_set_policy(0, 0.5, 0.0, 1.0)
    for groups in GROUPS:
        for lanes, depth, steps in LANES:
            for seed in SEEDS:
                L.p3host_selfplay_set_groups(groups)
                L.p3host_selfplay_set_lanes(lanes, depth)
                L.p3host_selfplay_set_step_limit(steps * groups)
                st, err = Stats(), C.create_string_buffer(256)
                rc = L.p3host_selfplay_run(b"hash", None, 0, GAMES * groups, 4, 16, 4, 16, 4, 24, 0.0, 1, seed, C.byref(st), err)
                assert rc == 0, err.value
                n = GAMES * groups
                out = (C.c_uint64 * n)()
                assert L.p3host_selfplay_last_first_game_digests(out, n) == n
                print(f"groups {groups} lanes {lanes} depth {depth} seed {seed} steps {steps * groups}: positions {st.positions} "
                      f"batches {st.batches} moves {st.moves} games {st.games}")
                for g in range(groups):
                    print("  " + " ".join(f"{d:016x}" for d in out[g * GAMES:(g + 1) * GAMES]))


def parse(text):
    """{(groups, lanes, depth, seed): (counters, [digests of group 0, of group 1, ...])}"""
    runs, key = {}, None
    for line in text.splitlines():
        w = line.split()
        if line.startswith("groups"):
            key = (int(w[1]), int(w[3]), int(w[5]), int(w[7].rstrip(":")))
            runs[key] = (tuple(int(w[i]) for i in (11, 13, 15, 17)), [])
        elif line.startswith("  "):
            runs[key][1].append([int(d, 16) for d in w])
    return runs


def main():
    if sys.argv[1] == "--run":
        return run_all(sys.argv[2])
    texts = []
    for title, path in zip(("parent", "branch"), sys.argv[1:3]):
        texts.append(subprocess.run([sys.executable, __file__, "--run", path], check=True, capture_output=True, text=True).stdout)
        print(f"==== {title}\n{texts[-1]}")
    a, b = parse(texts[0]), parse(texts[1])
    assert a.keys() == b.keys() and len(a) == len(GROUPS) * len(LANES) * len(SEEDS)
    bad = 0
    print("==== comparison (per run and group: first games finished in both builds / of those, equal digests)")
    for key in a:
        cells = []
        for da, db in zip(a[key][1], b[key][1]):
            both = [(x, y) for x, y in zip(da, db) if x and y]
            same = sum(x == y for x, y in both)
            cells.append(f"{len(both)}/{same}")
            bad += len(both) < 40 or same != len(both)
        note = ""
        if key[0] == 1 and key[1] == 1:
            eq = a[key][0] == b[key][0]
            bad += not eq
            note = f"  counters {'equal' if eq else 'DIFFER'} {a[key][0]}"
        print(f"groups {key[0]} lanes {key[1]} depth {key[2]} seed {key[3]}: {' '.join(cells)}{note}")
    print("ok" if not bad else f"FAILED: {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
