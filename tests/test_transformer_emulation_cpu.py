"""CPU checks of tests/tfm_emulation.py: the float64 mode against tfm_restatement_dh and the committed fixtures, the
twin against the kernel checker (this is where tfm_emulation.TWIN, and by its rule BOUNDS, come from), the hot regime
against the conditions it is there for, and the checker's power: each slip injected into the twin must fail it, naming
the kernel, the block and the place.  The whole module takes about a minute on 16 CPUs."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tfm_emulation as T  # noqa: E402
import tfm_restatement_dh as dh  # noqa: E402
import trunk_emulation as te  # noqa: E402
from conftest import load_golden  # noqa: E402

torch.set_num_threads(min(16, os.cpu_count() or 1))

NETS = list(dh.QK_SCALES)          # the eight transformer fixtures
D64 = [n for n in NETS if n in ("test_b2d128h2_tfm", "test_b2d256h4_tfm", "test_b2d384h6_tfm")]


def _net(name, hot=False):
    cfg, W = T.hot_weights(name) if hot else dh.fixture_weights(name)
    return cfg, W, load_golden(name)


def _hold_to_twin_table(fam):
    """the twin stays at or inside the figures BOUNDS were derived from (and so inside BOUNDS by their margin)"""
    for f, (ident, err) in fam.items():
        if f == "stem":
            continue
        assert err <= T.TWIN[f][0] + 1e-3 and ident >= T.TWIN[f][1] - 1e-4, (f, err, ident, T.TWIN[f])


def test_bounds_follow_the_rule():
    assert set(T.BOUNDS) == {f + h for f in ("qkv", "attn_d32", "attn_d64", "ffn_small", "ffn_wide") for h in ("", " hot")}
    for f, (err, ident) in T.TWIN.items():
        b = T.BOUNDS[f]
        assert b[0] % 0.5 == 0 and 2 * err <= b[0] < 2 * err + 0.5 and abs(b[1] - (ident - 0.05)) <= 1e-3, (f, b)


@pytest.mark.parametrize("name", NETS)
def test_float64_mode_is_the_restatement(name):
    """Chained: the raw outputs equal tfm_restatement_dh.forward's bit for bit and the committed fixture's to its
    float32 storage.  Kernel by kernel from the restatement's own tensors: each entry point equals its stage, and the
    kernel's softmax forms (exp2 of scaled scores over 384 keys with 23 masked; whole row, and online over blocks of
    64 keys) equal the plain softmax to float64 rounding."""
    cfg, W, (g, pos) = _net(name)
    n = min(len(pos), 4)
    planes, sc = te.inputs(pos[:n])
    assert np.array_equal(planes, g["planes"][:n].astype(np.float32)) and np.array_equal(sc, g["scalars"][:n])
    emu = T.Tfm(cfg, W, fp16=False)
    rec = emu.trunk(pos[:n])
    ref = dh.forward(cfg, W, planes, sc)
    assert np.array_equal(rec["x"][-1].numpy(), ref["trunk"])
    raw = emu.heads(rec["x"][-1])
    assert np.array_equal(raw, ref["raw"])
    want = g["raw"][:n].astype(np.float64)
    assert (np.abs(raw - want) <= 1e-9 + 2.0 ** -24 * np.abs(want)).all(), np.abs(raw - want).max()
    for i in range(cfg.blocks):
        x = rec["x"][i]
        q, k, v = dh.qkv_stage(x, W, i, cfg.bottleneck_channels)
        for a, b in zip(emu.qkv(i, x), (q, k, v)):
            assert torch.equal(a, b.permute(0, 2, 1, 3))
        o = dh.attn_stage(q, k, v)
        assert torch.equal(emu.attn(rec["q"][i], rec["k"][i], rec["v"][i]), o)
        for online in (False, True):
            o2 = emu.attn_kernel(rec["q"][i], rec["k"][i], rec["v"][i], online=online)[0]
            assert float((o2 - o).abs().max()) <= 1e-12 * max(1.0, float(o.abs().max())), (i, online)
        assert torch.equal(emu.ffn(i, o, x), dh.block(x, W, i, cfg.bottleneck_channels))


def test_fp16_mode_chained_is_the_restatements_fp16_mode():
    """At head width 32 the fp16 mode chained is tfm_restatement_dh.forward(fp16=True) bit for bit (head width 64
    differs by design: the online softmax's rounding, module docstring of tfm_emulation)."""
    cfg, W, (g, pos) = _net("test_b2d192h6_tfm")
    planes, sc = te.inputs(pos[:4])
    x = T.Tfm(cfg, W).trunk(pos[:4])["x"][-1]
    assert np.array_equal(x.numpy(), dh.forward(cfg, W, planes, sc, fp16=True)["trunk"])


@pytest.mark.parametrize("hot", [False, True], ids=["plain", "hot"])
@pytest.mark.parametrize("name", NETS)
def test_twin_passes_the_checker(name, hot):
    """The twin chained through the trunk on every fixture position, every kernel checked from the twin's own
    tensors, as the GPU test checks the engine: inside every bound, and at or inside tfm_emulation.TWIN."""
    cfg, W, (g, pos) = _net(name, hot)
    tw = T.Tfm(cfg, W, twin=True).trunk(pos)
    fam = T.collect({}, cfg, T.teacher_forced(T.Tfm(cfg, W), tw, pos, label=f"{name} block ", hot=hot), hot)
    print(name, {f: (round(e, 2), round(i, 4)) for f, (i, e) in fam.items()})
    _hold_to_twin_table(fam)


def test_twin_on_the_gpu_test_batches():
    """The twin in place of the engine on every job of test_transformer_blocks_gpu.py (its batches, sampled slots and
    hand-made positions, the hot nets among them)."""
    import test_transformer_blocks_gpu as G
    fam: dict = {}
    for name, batch in G.PLAIN_JOBS + G.HOT_JOBS:
        if name.endswith(":m1"):
            continue
        cfg, W, _ = G._weights(name)
        pos, slots, _ = G._batch(name, batch)
        hot = name.endswith(":hot")
        tw = T.Tfm(cfg, W, twin=True).trunk(pos[slots])
        T.collect(fam, cfg, T.teacher_forced(T.Tfm(cfg, W), tw, pos[slots], slots=slots, label=f"{name} block ", hot=hot), hot)
    print({f: (round(e, 2), round(i, 4)) for f, (i, e) in sorted(fam.items())})
    _hold_to_twin_table(fam)


def _hot_jobs():
    import test_transformer_blocks_gpu as G
    return [(n, b) for n, b in G.HOT_JOBS if n.endswith(":hot")]


def test_gpu_jobs_cover_what_the_issue_names():
    import test_transformer_blocks_gpu as G
    from p3achygo_amd import netspec
    assert {n for n, _ in G.PLAIN_JOBS} == set(NETS)
    assert {b for _, b in G.PLAIN_JOBS} >= {1, 7, 61, 300}
    cover = set()
    for n, _ in _hot_jobs():
        cfg = netspec.get_config(n.partition(":")[0])
        d = cfg.channels
        cover.add((d // cfg.bottleneck_channels, d <= 96, 128 if d <= 128 else (256 if d <= 256 else 384)))
    have = set()
    for n in NETS:      # every (attention path, FFN path, stream width) a fixture has is run hot
        cfg = netspec.get_config(n)
        d = cfg.channels
        have.add((d // cfg.bottleneck_channels, d <= 96, 128 if d <= 128 else (256 if d <= 256 else 384)))
    assert cover == have, have - cover
    assert {c[0] for c in cover} == {32, 64} and {c[1] for c in cover} == {True, False} and {c[2] for c in cover} == {128, 256, 384}
    assert sum(n.endswith(":m1") for n, _ in G.HOT_JOBS) == 1


@pytest.mark.parametrize("name", NETS[:1] + NETS[2:])
def test_hot_regime_is_what_it_claims(name):
    """On the emulation, block 0, the fixture positions (the nets of every hot GPU job and d = 64): peaked attention,
    most numerators below fp16's range, maxima beside the masked padding keys, the online softmax really rescaling;
    nothing overflows."""
    cfg, W, (g, pos) = _net(name, hot=True)
    emu = T.Tfm(cfg, W)
    rec = emu.trunk(pos[:8])
    reg = T.attention_regime(emu, rec["q"][0], rec["k"][0])
    top = max(float(x.abs().max()) for x in rec["x"])
    plain = T.Tfm(*dh.fixture_weights(name))
    prec = plain.trunk(pos[:8])
    print(name, "hot", {k: round(v, 3) for k, v in reg.items()}, f"max |x| {top:.1f}; plain",
          {k: round(v, 3) for k, v in T.attention_regime(plain, prec["q"][0], prec["k"][0]).items()})
    assert reg["peak"] >= 0.7 and reg["tiny"] >= 0.8 and reg["late"] >= 0.05, reg
    if emu.D == 64:
        assert reg["step8"] >= 0.4, reg
    for key in ("x", "q", "k", "v", "o"):
        assert all(bool(torch.isfinite(a).all()) for a in rec[key])
    assert top < 4096


@pytest.mark.parametrize("name", D64)
def test_online_softmax_form_is_not_the_row_maximum_form(name):
    """Head width 64: the kernel's form (numerators rounded against the running maximum of their block, rescaled in
    fp32) against one rounding against the row's maximum, on the same q, k, v, in the checker's measure.  Measured:
    never more than one rounding of o apart (max err 0.85 plain, 0.81 hot), but in 6.6 - 8.4 % of the elements on the
    fixtures and 2.7 - 2.9 % hot (peaked rows are carried by one key, so the small numerators matter less there, not
    more): with the row-maximum form as its emulation a correct kernel would miss attn_d64's fraction bit-identical
    on the plain fixtures.  So the emulation does what the kernel does."""
    for hot in (False, True):
        cfg, W, (g, pos) = _net(name, hot)
        emu = T.Tfm(cfg, W)
        r = emu.trunk(pos[:8])
        worst, ident = 0.0, 1.0
        for i in range(cfg.blocks):
            a = emu.attn_kernel(r["q"][i], r["k"][i], r["v"][i], online=True)[0]
            b = emu.attn_kernel(r["q"][i], r["k"][i], r["v"][i], online=False)[0]
            st = T.check_kernel("k_tfm_attn", "o", i, b, a, te.rms(a), 64, bound=(np.inf, 0.0))
            worst, ident = max(worst, st["max_err"]), min(ident, st["identical"])
        print(f"{name} {'hot' if hot else 'plain'}: row-maximum form against the online form: max err {worst:.2f}, "
              f"identical {ident:.4f}")
        assert worst <= 1.0, worst                       # one rounding of o
        assert ident < 0.99                              # and not the same function
        if not hot:
            assert ident < T.BOUNDS["attn_d64"][1], ident


@pytest.mark.parametrize("name", ["test_b2d96h3_tfm", "test_b2d256h4_tfm"])
def test_subnormal_switch_is_visible_to_the_checker(name):
    """flush_subnormals (MFMA operands below 2^-14 read as zero) against the default on the same q, k, v: outside the
    attention bounds on the fixtures and hot, so a GPU that passes with one setting did not compute the other."""
    for hot in (False, True):
        cfg, W, (g, pos) = _net(name, hot)
        emu = T.Tfm(cfg, W)
        r = emu.trunk(pos[:8])
        a = emu.attn(r["q"][0], r["k"][0], r["v"][0])
        b = T.Tfm(cfg, W, flush_subnormals=True).attn(r["q"][0], r["k"][0], r["v"][0])
        st = T.check_kernel("k_tfm_attn", "o", 0, b, a, te.rms(a), emu.D, bound=(np.inf, 0.0))
        print(f"{name} {'hot' if hot else 'plain'}: flushed against honoured subnormals: max err {st['max_err']:.2f}, "
              f"identical {st['identical']:.4f}")
        assert st["identical"] < T.BOUNDS[T.family(cfg, "attn", hot)][1]


def _tokens_over(msg):
    m = re.search(r"tokens over the bound (\d+)\.\.(\d+)", msg)
    return (int(m.group(1)), int(m.group(2))) if m else None


# (fixture, hot, mutation, what the message must start with after "block <net> block ", words it must contain,
# the token range the tokens over the bound must lie in or None)
MUTATIONS = [
    ("test_b2d96h3_tfm", False, dict(kind="K360", head=0), "0 k_tfm_attn o", ["heads over the bound [0]"], (352, 360)),
    ("test_b2d256h4_tfm", False, dict(kind="K360", head=2), "0 k_tfm_attn o", ["heads over the bound [2]"], (352, 360)),
    ("test_b2d96h3_tfm", False, dict(kind="PADKEY", key=361), "0 k_tfm_attn o", [], None),
    ("test_b2d256h4_tfm", True, dict(kind="PADKEY", key=383), "0 k_tfm_attn o", [], None),
    ("test_b2d96h3_tfm", False, dict(kind="KSHIFT"), "0 k_tfm_attn o", [], None),
    ("test_b2d256h4_tfm", True, dict(kind="KSHIFT"), "0 k_tfm_attn o", [], None),
    ("test_b2d192h6_tfm", False, dict(kind="ROPESWAP", block=1, head=4), "1 k_tfm_qkv q", ["heads over the bound [4]"], None),
    ("test_b2d96h3_tfm", False, dict(kind="WTILE", block=1, weight="q", tile=2), "1 k_tfm_qkv q",
     ["heads over the bound [1]", "groups [4, 5] "], None),
    ("test_b2d256h4_tfm", False, dict(kind="WTILE", block=0, weight="o", tile=1), "0 k_tfm_ffn x", [], None),
    ("test_b2d384h12_tfm", False, dict(kind="WTILE", block=1, weight="ffn_down", tile=22), "1 k_tfm_ffn x",
     ["groups [44, 45] "], None),
    ("test_b2d256h4_tfm", True, dict(kind="NORESCALE"), "0 k_tfm_attn o", [], None),
    ("test_b2d256h4_tfm", False, dict(kind="NORESCALE"), "0 k_tfm_attn o", [], None),
    ("test_b2d256h4_tfm", True, dict(kind="ALPHA0"), "0 k_tfm_attn o", [], None),
    ("test_b2d256h4_tfm", False, dict(kind="ALPHA0"), "0 k_tfm_attn o", [], None),
    ("test_b2d96h3_tfm", False, dict(kind="EPS", block=0, norm="in"), "0 k_tfm_qkv q", ["identical"], None),
    ("test_b2d256h4_tfm", False, dict(kind="EPS", block=0, norm="in"), "0 k_tfm_qkv q", ["identical"], None),
    ("test_b2d96h3_tfm", False, dict(kind="SILUSWAP", block=1, tile=3), "1 k_tfm_ffn x", [], None),
    ("test_b2d128h2_tfm", False, dict(kind="SILUSWAP", block=0, tile=15), "0 k_tfm_ffn x", [], None),
    ("test_b2d96h3_tfm", False, dict(kind="ROPEROW", block=1), "1 k_tfm_qkv q", [], (0, 63)),
]


def _mid(m):
    n, hot, mut = m[0], m[1], m[2]
    return f"{mut['kind']}{'-' + mut.get('weight', mut.get('norm', '')) if mut['kind'] in ('WTILE', 'EPS') else ''}-{n}{'-hot' if hot else ''}"


@pytest.mark.parametrize("name,hot,mut,where,words,tok", MUTATIONS, ids=[_mid(m) for m in MUTATIONS])
def test_checker_catches_mutation(name, hot, mut, where, words, tok):
    """teacher_forced checks stem, then per block qkv (q, k, v), attn, ffn, and raises at the first tensor outside its
    bound: a message that starts at the mutated kernel means every step in front of it passed."""
    cfg, W, (g, pos) = _net(name, hot)
    pos = pos[:8]
    tw = T.Tfm(cfg, W, twin=True, mutate=mut).trunk(pos)
    with pytest.raises(AssertionError) as exc:
        T.teacher_forced(T.Tfm(cfg, W), tw, pos, label=f"{name} block ", hot=hot)
    msg = str(exc.value)
    print(msg)
    assert msg.startswith(f"block {name} block {where}:") and all(w in msg for w in words), msg
    if tok is not None:
        got = _tokens_over(msg)
        assert got is not None and tok[0] <= got[0] and got[1] <= tok[1], (got, msg)
    if mut["kind"] == "ROPEROW":
        assert "slots [1, " in msg      # position 0 starts at a tile boundary: only later positions have such tokens
    if mut["kind"] == "K360":
        _report_k360(name, cfg, W, tw, g)


def _report_k360(name, cfg, W, tw, g):
    """Information only: the output-level bounds of test_transformer_gpu.py / test_transformer_widths_gpu.py let the
    twin with the lost key through."""
    from test_transformer_gpu import LOGIT_REL, TOL
    from test_transformer_widths_gpu import TOL as TOL_W
    tol = {**TOL_W, **TOL}[name]["logit"]
    raw = T.Tfm(cfg, W, twin=True).heads(tw["x"][-1])
    want = g["raw"][:len(raw)].astype(np.float64)
    ok = (np.abs(raw - want) <= np.maximum(tol, LOGIT_REL * np.abs(want))).all()
    clean = T.Tfm(cfg, W, twin=True).forward(load_golden(name)[1][:len(raw)])
    print(f"K360 replay on {name}: max |d| of the raw outputs against the fixture {np.abs(raw - want).max():.2e} "
          f"(clean twin {np.abs(clean - want).max():.2e}, bound {tol:.2e}): the output-level bound would "
          f"{'NOT ' if ok else ''}have flagged it")


def test_rescale_faults_are_caught_plain_and_hot():
    """Measured, not assumed: the online softmax without its rescale of o is no finding of the hot jobs.  The running
    maximum moves by a little in most rows of the plain fixtures as well, and the checker rejects NORESCALE there by
    four orders of magnitude (4.0e4 plain, 2.1e4 hot).  Even a rescale that only fails for large steps (ALPHA0: alpha
    below 2^-8 taken for 0) is rejected on both (27 plain, 32 hot), through the 0.1 - 0.2 % of plain rows that take
    such a step; hot it is 50 - 62 % of the rows.  What the hot jobs add is the regime itself (subnormal and flushed
    P operands, real rescaling in most rows), not a mutant only they can see."""
    name = "test_b2d256h4_tfm"
    err, rows = {}, {}
    for hot in (False, True):
        cfg, W, (g, pos) = _net(name, hot)
        emu = T.Tfm(cfg, W)
        r = emu.trunk(pos[:8])
        good = emu.attn(r["q"][0], r["k"][0], r["v"][0])
        rows[hot] = T.attention_regime(emu, r["q"][0], r["k"][0])["step8"]
        for kind in ("NORESCALE", "ALPHA0"):
            bad = T.Tfm(cfg, W, mutate=dict(kind=kind)).attn_kernel(r["q"][0], r["k"][0], r["v"][0])[0]
            err[kind, hot] = T.check_kernel("k_tfm_attn", "o", 0, bad, good, te.rms(good), 64,
                                            bound=(np.inf, 0.0))["max_err"]
    print({f"{k} {'hot' if h else 'plain'}": round(v, 2) for (k, h), v in err.items()}, "rows with a step >= 8:", rows)
    assert err["NORESCALE", False] > 100 and err["NORESCALE", True] > 100
    assert err["ALPHA0", False] > T.BOUNDS["attn_d64"][0] and err["ALPHA0", True] > T.BOUNDS["attn_d64 hot"][0]
    assert rows[False] < 0.01 and rows[True] >= 0.4
