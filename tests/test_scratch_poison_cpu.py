"""No device buffer of the engine without a decision on what a forward pass may read of it: the table p3hip_debug_poison
goes by (csrc/engine.cpp kDeviceBuffers, read through p3hip_debug_poison_table, no device needed) against struct
p3hip_engine as csrc/engine.h declares it.  tests/test_scratch_poison_gpu.py is what the hook is for.

The rule for "device pointer member": inside `struct p3hip_engine { ... }`, its nested structs included, every declarator
of pointer type whose name starts with d_ (comments and preprocessor lines taken out first, so the members of the
diagnostic build count too).  A member of a nested struct is named by the nested struct's member name, as the code
reaches it: cache.d_tkeys, scoring.d_rows, loss.d_rows.  That the d_ prefix is the whole set is itself checked: every
hipMalloc of the engine's sources must name one of the members found.
"""
import glob
import os
import re

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")
CLASSES = {"poisoned", "state", "index", "zeroed-once"}
# what the issue of the hook fixes: these are filled, these never are
MUST_POISON = {"d_x", "d_t", "d_u", "d_s", "d_hp", "d_pool", "d_cout", "d_out", "d_res", "d_aux",
               "scoring.d_terms", "scoring.d_sums", "loss.d_terms", "loss.d_sums"}
MUST_KEEP = {"d_arena": "state", "d_amax": "state", "d_ascale": "state", "cache.d_tkeys": "state", "cache.d_tmeta": "state",
             "cache.d_tvals": "state", "scoring.d_labels": "state", "loss.d_targets": "state",
             "d_feats": "index", "d_sfeats": "index", "cache.d_feats2": "index", "d_symtab": "index", "cache.d_keys": "index",
             "cache.d_hit": "index", "cache.d_victim": "index", "cache.d_lists": "index", "scoring.d_rows": "index",
             "loss.d_rows": "index"}


def _strip(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))


def device_pointer_members(header_text):
    """[qualified name] of the device pointer members of struct p3hip_engine, nested structs first, repeats kept"""
    text = _strip(header_text)
    start = re.search(r"\bstruct\s+p3hip_engine\s*\{", text)
    assert start, "struct p3hip_engine not found"
    depth, i = 1, start.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    body = text[start.end():i - 1]
    found = []

    def scan(chunk, prefix):
        # nested structs first: `struct Name { ... } member;`
        pos, flat = 0, ""
        for m in re.finditer(r"\bstruct\s+\w+\s*\{", chunk):
            if m.start() < pos:
                continue
            d, j = 1, m.end()
            while d:
                d += {"{": 1, "}": -1}.get(chunk[j], 0)
                j += 1
            member = re.match(r"\s*(\w+)\s*;", chunk[j:])
            assert member, "a nested struct of p3hip_engine without a member name"
            flat += chunk[pos:m.start()]
            scan(chunk[m.end():j - 1], prefix + member.group(1) + ".")
            pos = j + member.end()
        flat += chunk[pos:]
        # member functions' bodies hold no members
        flat = re.sub(r"\{[^{}]*\}", ";", flat)
        for decl in flat.split(";"):
            for name in re.findall(r"\*\s*(d_\w+)", decl):
                found.append(prefix + name)

    scan(body, "")
    return found


@pytest.fixture(scope="module")
def table(built):
    from p3achygo_amd import engine
    return engine.debug_poison_table()


@pytest.fixture(scope="module")
def members():
    return device_pointer_members(open(os.path.join(CSRC, "engine.h")).read())


def test_the_parser_finds_nested_and_conditional_members(members):
    assert len(members) == len(set(members)), sorted(m for m in members if members.count(m) > 1)
    for name in ("d_x", "d_qkv", "d_stamps", "d_spans", "d_bw_stamps", "cache.d_feats2", "scoring.d_rows", "loss.d_rows",
                 "d_symtab", "d_cout"):
        assert name in members, name
    assert not any(m.split(".")[-1].startswith("h_") for m in members)
    # the parser itself, on a struct it has not seen
    toy = """struct p3hip_engine { int* a = nullptr; float *d_a = nullptr, *h_b, *d_b;   // float* d_no;
      #ifdef X
      char* d_c;
      #endif
      /* int* d_never; */ const int* f() const { return (const int*)d_a; }
      struct In { unsigned *h_q = nullptr, *d_q = nullptr; std::vector<int*> d_vec; } in; };"""
    assert device_pointer_members(toy) == ["in.d_q", "d_a", "d_b", "d_c"]


def test_every_device_pointer_has_exactly_one_class(table, members):
    """engine.debug_poison_table raises on a member with two rows; here: the same set, every class a known one"""
    assert set(table) == set(members), {"without a row": sorted(set(members) - set(table)),
                                         "rows without a member": sorted(set(table) - set(members))}
    for name, (cls, zero_range) in table.items():
        assert cls in CLASSES, (name, cls)
        assert bool(zero_range) == (cls == "zeroed-once"), (name, cls, zero_range)


def test_the_classes_the_hook_was_built_for(table):
    assert {n for n, (c, _) in table.items() if c == "poisoned"} >= MUST_POISON
    for name, cls in MUST_KEEP.items():
        assert table[name][0] == cls, (name, table[name])
    assert table["d_qkv"] == ("zeroed-once", "token rows 361..383 of every head of q, k and v")
    assert [n for n, (c, _) in table.items() if c == "zeroed-once"] == ["d_qkv"]


def test_every_device_allocation_is_a_member_the_rule_finds(members):
    """the d_ prefix is the whole set: each hipMalloc of the engine's host sources allocates one of the members"""
    last = {m.split(".")[-1] for m in members}
    seen = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.cpp"))):
        for target in re.findall(r"\bhipMalloc\(\s*\(void\*\*\)\s*&\s*([\w.>-]+)", open(path).read()):
            name = re.split(r"\.|->", target)[-1]
            assert name in last, (os.path.basename(path), target)
            seen.add(name)
    assert {"d_x", "d_tkeys", "d_terms", "d_bw_stamps", "d_stamps"} <= seen   # the search itself finds them


def test_the_hook_is_declared_exported_and_mirrored(built):
    from p3achygo_amd import engine
    hdr = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    assert re.search(r"\bint p3hip_debug_poison\(p3hip_engine\* e, int byte\);", hdr)
    assert re.search(r"\bconst char\* p3hip_debug_poison_table\(void\);", hdr)
    assert {"p3hip_debug_poison", "p3hip_debug_poison_table"} <= set(engine.EXPORTS)
    assert callable(engine.HipEngine.debug_poison)
    for name in ("p3hip_debug_poison", "p3hip_debug_poison_table"):
        getattr(engine.lib(), name)
