"""What the host-side plan (csrc/plan.cpp) decides and packs, cell by cell, against tests/golden/plan_matrix.json.

Two tables, both made with tools/plan_sanitize_main.cpp, a stand-alone program over csrc/plan.h that this test builds
once per session (host code only) and runs as a child process with the cell's P3HIP_* environment:

 (a) the decision grid: choose_plan alone (--choose) on files that are only a header, over trunk shapes x flag sets x
     environment switches: the full refusal text, or the Path and the PlanChoice fields;
 (b) the arena table: build_plan on seeded weights: path, blocks, layers, quantized tensors, the arena's size and the
     FNV-1a digest of its bytes.  The order of Arena::add calls is behaviour (plan.h), and the digest pins it.

The golden file is recorded with THIS tool source built against a checkout of the commit whose behaviour is to be kept
(its hash goes into the file), never from the tree under test: copy tools/plan_sanitize_main.cpp into that checkout
(it uses nothing of plan.h that the commit before it lacks), and there
    hipcc -O1 -std=c++17 -x hip --offload-arch=gfx950 --offload-host-only tools/plan_sanitize_main.cpp \\
        p3achygo_amd/csrc/plan.cpp -o /tmp/plan_tool
then here
    python tests/test_plan_matrix_cpu.py --record /tmp/plan_tool <commit hash>
"""
import itertools
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conftest import ROOT  # noqa: E402
from test_create_matrix_cpu import NETS as CREATE_NETS  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_matrix.json")
CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")
TOOL_SRC = os.path.join(ROOT, "tools", "plan_sanitize_main.cpp")

PLAN_FLAGS = ["INT8", "INT8_FUSED", "INT8_C128", "INT8_ANY", "FP32", "FP32_TFM", "LOW_LATENCY"]
GRID_FLAG_SETS = (["0"] + PLAN_FLAGS + [a + " | " + b for a, b in itertools.combinations(PLAN_FLAGS, 2)] +
                  ["FP32 | FP32_TFM | INT8", "INT8 | INT8_FUSED | INT8_C128", " | ".join(PLAN_FLAGS)])
GRID_ENVS = ["", "P3HIP_CONV_ANY=1", "P3HIP_BLOCKW=1", "P3HIP_NO_HFUSE=1", "P3HIP_SPLIT=2,32", "P3HIP_SPLIT=3,64"]
WIDTHS = [(256, 128), (128, 64), (384, 192), (64, 32), (96, 48), (192, 96), (256, 256), (512, 128), (320, 160), (256, 24),
          (40, 16), (544, 128)]
TFMS = [(64, 2), (96, 3), (128, 2), (256, 4), (384, 6), (384, 12), (96, 2), (416, 13)]

ARENA_NETS = CREATE_NETS + ["test_b3c512nbt", "test_b3c192btl3"]
ARENA_FLAG_SETS = ["0"] + PLAN_FLAGS
AUX_NETS = ["test_b3c256btl1", "test_b2d96h3_tfm"]

# each refusal of choose_plan, by a piece of its text that no other has
REFUSALS = [
    "P3HIP_FLAG_LOW_LATENCY serves the conv trunks",
    "P3HIP_FLAG_LOW_LATENCY cannot be combined with P3HIP_FLAG_INT8,",
    "P3HIP_FLAG_LOW_LATENCY cannot be combined with P3HIP_FLAG_FP32 ",
    "P3HIP_FLAG_LOW_LATENCY: P3HIP_SPLIT must be",
    "P3HIP_FLAG_INT8_ANY serves the conv trunks",
    "P3HIP_FLAG_INT8_ANY cannot be combined with P3HIP_FLAG_INT8,",
    "P3HIP_FLAG_INT8_ANY cannot be combined with P3HIP_FLAG_FP32 ",
    "P3HIP_FLAG_FP32 serves the conv trunks only",
    "P3HIP_FLAG_FP32_TFM serves the transformer trunks only",
    "C128: an engine runs one precision plan",
    "unsupported architecture for the HIP engine",
    "INT8_C128 is available only for",
    " is not available for this conv trunk",
    "INT8_FUSED is available only for",
    "INT8 is available only for layer-wise trunks",
]
PATHS = ["Fused", "Blockw", "Layerwise", "ConvAny", "Int8", "Int8Fused256", "Int8Fused128", "Int8Any", "F32Conv", "Split",
         "Tfm", "TfmF32"]


def _flags(names):
    from p3achygo_amd import engine
    return sum(getattr(engine, "FLAG_" + n.strip()) for n in names.split("|") if n.strip() != "0")


def grid_headers():
    """name -> (C, C_b or heads, H, V, broadcast interval, inner, block type) of the header-only files of table (a)"""
    out = {}
    for C, Cb in WIDTHS:
        for bint in (1, 2, 3):
            for inner in range(5):
                out[f"c{C}b{Cb}btl{inner}_i{bint}"] = (C, Cb, 32, 64, bint, inner, "btl")
            out[f"c{C}b{Cb}nbt_i{bint}"] = (C, Cb, 32, 64, bint, 2, "nbt")
    for C in (64, 96, 128, 192, 512):
        for inner in (2, 3):
            out[f"c{C}classic{inner}"] = (C, C // 2, 32, 64, 3, inner, "classic")
    for d, heads in TFMS:
        out[f"d{d}h{heads}tfm"] = (d, heads, 32, 64, 0, 0, "transformer")
    for V in (32, 48, 64, 80, 96):
        for H in (32, 64):
            out[f"c256b128btl3_i3_H{H}V{V}"] = (256, 128, H, V, 3, 3, "btl")
            out[f"c384b192nbt_i3_H{H}V{V}"] = (384, 192, H, V, 3, 2, "nbt")
            out[f"d96h3tfm_H{H}V{V}"] = (96, 3, H, V, 0, 0, "transformer")
    return out


def write_header_file(path, C, Cb, H, V, bint, inner, btype):
    """magic, the ten ints and one one-float tensor: what WeightFile::load accepts and choose_plan needs"""
    from p3achygo_amd import netspec
    blob = netspec._HDR.pack(b"P3W1", 1, 4, C, Cb, H, V, bint, inner, netspec.BLOCK_TYPES[btype], 1)
    blob += netspec._ENT.pack(b"none", 1, 1, 1, 1, 1, 0)
    blob += b"\0" * ((-len(blob)) % 64)
    with open(path, "wb") as f:
        f.write(blob + b"\0\0\0\0")


def arena_envs(cfg):
    """the environments of table (b) whose switch the plan (or the launches over it) of this net reads"""
    C, Cb, bt = cfg.channels, cfg.bottleneck_channels, cfg.block_type
    fused = bt in ("btl", "nbt") and (C, Cb) in ((256, 128), (128, 64))
    envs = [""]
    if (bt in ("btl", "nbt") and (C, Cb) == (384, 192)) or (bt == "classic" and C == 192):
        envs.append("P3HIP_CONV_ANY=1")
    if bt == "btl" and (C, Cb) == (256, 128):
        envs += ["P3HIP_BLOCKW=1", "P3HIP_NO_DFUSE=1"]
    if fused:
        envs += ["P3HIP_NO_BFUSE=1", "P3HIP_NO_FUSE=1"]
    if fused and C == 128:
        envs.append("P3HIP_C128_WG8=1")
    return envs


def run_tool(tool, env, args, files, flag_sets):
    """the tool's answer for every (file, flag set), in that order, without the 'file: flags: ' in front"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("P3HIP_")}
    if env:
        k, v = env.split("=")
        e[k] = v
    flags = [_flags(fs) for fs in flag_sets]
    out = subprocess.run([tool] + args + [",".join(map(str, flags))] + files, env=e, check=True, capture_output=True,
                         text=True).stdout.splitlines()
    assert len(out) == len(files) * len(flags), out[-3:]
    cells = []
    for i, line in enumerate(out):
        head = f"{files[i // len(flags)]}: {flags[i % len(flags)]}: "
        assert line.startswith(head), line
        cells.append(line[len(head):])
    return cells


def tables(tool, directory):
    """(a) {env: {header: [outcome per GRID_FLAG_SETS]}} and (b) {net: {env: {flag set: outcome}}}"""
    from p3achygo_amd import netspec
    d = str(directory)
    headers = grid_headers()
    for name, h in headers.items():
        write_header_file(os.path.join(d, name + ".p3w"), *h)
    files = [os.path.join(d, n + ".p3w") for n in headers]
    n = len(GRID_FLAG_SETS)
    grid = {}
    for env in GRID_ENVS:
        cells = run_tool(tool, env, ["--choose"], files, GRID_FLAG_SETS)
        grid[env] = {name: cells[i * n:(i + 1) * n] for i, name in enumerate(headers)}
    arena = {}
    for net in ARENA_NETS:
        cfg = netspec.get_config(net)
        path = os.path.join(d, net + ".p3w")
        netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=True))
        fsets = ARENA_FLAG_SETS + (["AUX"] if net in AUX_NETS else [])
        arena[net] = {env: dict(zip(fsets, run_tool(tool, env, [], [path], fsets))) for env in arena_envs(cfg)}
        os.remove(path)
    return grid, arena


def encode(grid, arena, parent):
    """distinct outcome strings once, distinct grid rows once; everything else refers to them by index"""
    outcomes, rows = [], []

    def idx(table, v):
        if v not in table:
            table.append(v)
        return table.index(v)
    g = {env: [idx(rows, [idx(outcomes, o) for o in grid[env][h]]) for h in grid[env]] for env in grid}
    a = {net: {env: {fs: idx(outcomes, o) for fs, o in cells.items()} for env, cells in envs.items()}
         for net, envs in arena.items()}
    return {"parent": parent, "outcomes": outcomes, "headers": list(grid[""]), "flag_sets": GRID_FLAG_SETS, "rows": rows,
            "grid": g, "arena": a}


def decode(gold):
    o = gold["outcomes"]
    grid = {env: {h: [o[k] for k in gold["rows"][r]] for h, r in zip(gold["headers"], rws)} for env, rws in gold["grid"].items()}
    arena = {net: {env: {fs: o[k] for fs, k in cells.items()} for env, cells in envs.items()}
             for net, envs in gold["arena"].items()}
    return grid, arena


def _build(out):
    subprocess.run(["hipcc", "-O1", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "--offload-host-only", TOOL_SRC,
                    os.path.join(CSRC, "plan.cpp"), "-o", out], check=True, capture_output=True, text=True)
    return out


@pytest.fixture(scope="session")
def plan_tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_matrix")
    return tables(_build(os.path.join(str(d), "plan_tool")), d)


@pytest.fixture(scope="session")
def golden():
    gold = json.load(open(GOLDEN))
    return gold, decode(gold)


def test_the_golden_grid_reaches_every_path_and_every_refusal(golden):
    gold, (grid, arena) = golden
    assert len(gold["parent"]) == 40
    assert gold["headers"] == list(grid_headers()) and gold["flag_sets"] == GRID_FLAG_SETS and sorted(grid) == sorted(GRID_ENVS)
    seen = {o for env in grid for row in grid[env].values() for o in row}
    for p in PATHS:
        assert any(o.startswith(p + ", ") for o in seen), p
    for r in REFUSALS:
        assert any(o.startswith("refused: ") and r in o for o in seen), r
    # distinct texts: "cannot be combined with P3HIP_FLAG_INT8, .." begins with FP32, FP32_TFM or both, "is not available
    # for this conv trunk" with INT8 or INT8_FUSED
    assert len({o for o in seen if o.startswith("refused: ")}) == len(REFUSALS) + 2 + 1
    assert sorted(arena) == sorted(ARENA_NETS)


def test_every_plan_decision_is_the_recorded_one(plan_tables, golden):
    got, want = plan_tables[0], golden[1][0]
    wrong = [(env, h, fs, g, w) for env in GRID_ENVS for h in want[env]
             for fs, g, w in zip(GRID_FLAG_SETS, got[env][h], want[env][h]) if g != w]
    assert not wrong, (len(wrong), wrong[:10])


def test_every_arena_is_the_recorded_one(plan_tables, golden):
    got, want = plan_tables[1], golden[1][1]
    assert {n: sorted(e) for n, e in got.items()} == {n: sorted(e) for n, e in want.items()}
    wrong = [(net, env, fs, got[net][env].get(fs), w) for net in want for env in want[net] for fs, w in want[net][env].items()
             if got[net][env].get(fs) != w]
    assert not wrong, (len(wrong), wrong[:10])


if __name__ == "__main__" and len(sys.argv) == 4 and sys.argv[1] == "--record":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        json.dump(encode(*tables(sys.argv[2], tmp), sys.argv[3]), open(GOLDEN, "w"), separators=(",", ":"))
        print("recorded", GOLDEN)
