"""The Winograd plan on the MI355X (P3HIP_FLAG_WINOGRAD).

The nets (winograd_restatement.NETS) are three or four blocks each and the smallest shapes at which k_wconv can go wrong:
one K slice (test_b3c64btl2), a padded C_b (test_b3c192btl3), both widths padded with the nbt res / dual flows
(test_b3c96nbt), the templated widths (test_b3c384btl3 / nbt), the prologue with C -> C (the classic nets), broadcast
blocks in between (test_b4c512btl3_i2).

Accuracy: block by block, teacher-forced, against the CPU emulation of the same scheme (tests/winograd_restatement.py)
run from the engine's own x, inside BLOCK_BOUNDS (set from the emulation's twin, not from the engine), at batch 3, at
batch 5 (the tiles of two positions in one unit of 32: 500 tiles are no multiple of 32 either) and at the first batch at
which a workgroup takes a second unit on this device; whole nets against the float64 outputs inside WHOLE_NET.  Everything
else is bit for bit.  Every step with more than one engine runs in a child process (tests/winograd_child.py) under its own
time limit; nothing is retried, and once a child failed no further one starts.

Measured on one MI355X (256 CUs; winograd_restatement.GPU_MEASURED): blocks, worst err / least identical, wino_btl 1.95 /
0.610, wino_nbt 4.18 / 0.462, wino_classic 3.49 / 0.493 (the twin: 2.12 / 0.600, 4.27 / 0.461, 3.51 / 0.492); whole nets
0.25 - 0.43 of their bounds in the raw outputs; the file takes 35 s, its longest test 5.4 s."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_widths_common as cw  # noqa: E402
import trunk_emulation as te  # noqa: E402
import winograd_restatement as wr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "winograd_child.py")
MECH_NET = "test_b3c96nbt"
CHILD_TIMEOUT = 240
HIP_ATTR_MULTIPROCESSOR_COUNT = 63         # hipDeviceAttributeMultiprocessorCount (hip/hip_runtime_api.h)


def _garbage_twin(cfg, W):
    """(cfg, W) zero-padded to multiples of 64 as the engine pads (conv_widths_common.pad_weights), then garbage (uniform
    in +-3) wherever a padded weight channel cannot reach a real value: the padded output columns of every conv whose
    output passes a BN (all but a block's last conv: the padded channel's folded BN is scale = shift = 0, so its
    activation is mish(0) = 0 whatever the conv gave) and the padded input rows of every conv that reads such a tensor,
    the 3x3 convs included: their V there is the transform of exact zeros."""
    rng = np.random.default_rng(5)
    C, Cb = cfg.channels, cfg.bottleneck_channels
    big, P = cw.pad_weights(cfg, W)
    for i in range(cfg.blocks):
        if cfg.block_kind(i) == "broadcast":
            continue
        n = cfg.inner_layers + 2
        for j in range(n):
            w = P[f"blocks.{i}.conv{j}.w"]   # [k][k][cin][cout]
            cin, cout = (C if j == 0 else Cb), (C if j == n - 1 else Cb)
            if j < n - 1:
                w[:, :, :cin, cout:] = rng.uniform(-3, 3, w[:, :, :cin, cout:].shape)
            w[:, :, cin:, :cout] = rng.uniform(-3, 3, w[:, :, cin:, :cout].shape)
    return big, P


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from p3achygo_amd import netspec
    d = tmp_path_factory.mktemp("winograd")
    cache = {}

    def get(name, garbage=False):
        key = (name, garbage)
        if key not in cache:
            cfg, W = wr.config(name), wr.weights(name)
            if garbage:
                cfg, W = _garbage_twin(cfg, W)
            cache[key] = os.path.join(d, name + ("_garbage" if garbage else "") + ".p3w")
            netspec.save_p3w(cache[key], cfg, W)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def n_cu(built):
    """CU count of device 0 as the engine's launchers see it (tests/test_batch_geometry_gpu.py)"""
    from p3achygo_amd import engine
    engine.lib()
    with open("/proc/self/maps") as f:
        hip = sorted({ln.split()[-1] for ln in f if "libamdhip64.so" in ln})
    assert hip, "libp3hip.so did not load the HIP runtime"
    rt = ctypes.CDLL(hip[0], mode=os.RTLD_NOLOAD | os.RTLD_GLOBAL)
    v = ctypes.c_int(0)
    assert rt.hipDeviceGetAttribute(ctypes.byref(v), HIP_ATTR_MULTIPROCESSOR_COUNT, 0) == 0
    assert v.value > 0
    return v.value


_FAILED = []


def _child(job, tmp, env_extra=None, **arrays):
    """One child process under its own time limit, nothing retried; once one failed no further one is started."""
    if _FAILED:
        pytest.fail("an earlier child failed: no further GPU process is started (%s)" % _FAILED[0])
    env = {k: v for k, v in os.environ.items()
           if k not in ("P3HIP_NO_HFUSE", "P3HIP_NO_FUSE", "P3HIP_NO_BFUSE", "P3HIP_DEBUG_STOP_BLOCK", "P3HIP_CONV_ANY")}
    env.update(env_extra or {})
    tag = job + ("_any" if env_extra else "")
    inp, outp = os.path.join(str(tmp), f"in_{tag}.npz"), os.path.join(str(tmp), f"out_{tag}.npz")
    np.savez(inp, **arrays)
    try:
        r = subprocess.run([sys.executable, CHILD, job, inp, outp], env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _FAILED.append("time limit")
        raise
    if r.returncode != 0:
        _FAILED.append("exit %d" % r.returncode)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(outp))


# ---- 1. blocks, teacher-forced ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", wr.NETS)
def test_blocks_teacher_forced(built, files, tmp_path, n_cu, name):
    """The engine's x after block k against the emulation of block k from the engine's x after block k - 1, by
    check_block (its failure message names corner / edge / interior: row and column 18 are the half-empty tiles) inside
    winograd_restatement.BLOCK_BOUNDS; broadcast blocks and the stem by trunk_emulation's own bounds, the stem bit for bit
    the fp16 engine's; padded channels of the stream exactly 0; the heads within HEADS_TOL on the engine's own x."""
    import torch
    from p3achygo_amd import engine
    from test_conv_widths_gpu import block_batch
    cfg, W = wr.config(name), wr.weights(name)
    C, Cp = cfg.channels, cw.padded(cfg.channels)
    second = wr.second_unit_batch(cfg, n_cu, lambda n, c: engine.debug_wconv_grid(n, c, n_cu))
    grid, units = engine.debug_wconv_grid(second, cw.padded(wr.conv3_width(cfg)), n_cu)
    assert units > grid == n_cu and second > 5
    batches = (3, 5, second)
    out = _child("blocks", tmp_path, path=np.array(files(name)), Cp=np.array(Cp), blocks=np.array(cfg.blocks),
                 batches=np.array(batches))
    emu = wr.WTrunk(cfg, W)
    worst = {}
    for batch in batches:
        pos, slots = block_batch(batch)
        full = [out[f"b{batch}:x{s}"] for s in range(cfg.blocks + 1)]
        assert np.abs(full[0]).max() > 0
        assert out[f"b{batch}:x0_fp16"].tobytes() == full[0].tobytes()
        for x in full:
            assert np.isfinite(x).all() and np.all(x[:, C:] == 0)
        xs = [x[:, :C] for x in full]
        st = wr.teacher_forced(emu, xs, pos[slots], slots=slots, label=f"{name} batch {batch} block ")
        for k, v in st.items():
            kind = "stem" if k == "stem" else wr.kind_of(cfg, k)
            a = worst.setdefault(kind, [0.0, 1.0])
            a[0], a[1] = max(a[0], v["max_err"]), min(a[1], v["identical"])
        want = emu.heads(torch.from_numpy(xs[-1].astype(np.float64).reshape(len(slots), C, 19, 19)))
        d = np.abs(out[f"b{batch}:raw"] - np.asarray(want))
        assert d.max() <= te.HEADS_TOL, (name, batch, float(d.max()))
    print(f"{name} batches {batches}:", {k: (round(a, 2), round(b, 3)) for k, (a, b) in worst.items()})


# ---- 2. whole nets ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", wr.NETS)
def test_whole_net_within_three_times_the_emulations_error_to_float64(built, files, name):
    """batch 16 (conv_widths_common.positions()): max |d| of the raw outputs, the move probabilities and the value
    probabilities to the float64 outputs within winograd_restatement.WHOLE_NET"""
    from p3achygo_amd import engine
    cfg, W = wr.config(name), wr.weights(name)
    pos = cw.positions()
    ref = cw.outputs(cfg, W, pos, fp16=False)
    eng = engine.HipEngine(files(name), 16, flags=engine.FLAG_WINOGRAD)
    eng.load_all(pos)
    eng.RunInference()
    res = [eng.GetBatch(s) for s in range(16)]
    got = {"raw": np.stack([eng.get_raw(s) for s in range(16)]),
           "move_probs": np.stack([np.ctypeslib.as_array(r.move_probs) for r in res]).astype(np.float64),
           "value_probs": np.stack([np.ctypeslib.as_array(r.value_probs) for r in res]).astype(np.float64)}
    eng.close()
    assert np.isfinite(got["raw"]).all()
    err = wr.errors(got, ref)
    print(f"{name}: {err} of {wr.WHOLE_NET[name]}")
    for k, bound in wr.WHOLE_NET[name].items():
        assert err[k] <= bound, (name, k, err)


# ---- 3. both forms of the 1x1 kernels; the plan is its own; the timing hook -------------------------------------------

@pytest.fixture(scope="module")
def forms(built, files, tmp_path_factory):
    """'own': the templated nets under the flag and test_b3c384btl3 in fp16, plus a classic and a padded net under the
    flag for the timing hook; 'any' (P3HIP_CONV_ANY=1): the templated nets under the flag"""
    from p3achygo_amd import engine
    tmp = tmp_path_factory.mktemp("forms")
    F = engine.FLAG_WINOGRAD
    jobs = {"own": [(n + ":wino", files(n), F) for n in wr.TEMPLATED + ("test_b3c128classic", "test_b3c96nbt")] +
                   [("test_b3c384btl3:fp16", files("test_b3c384btl3"), 0)],
            "any": [(n + ":wino", files(n), F) for n in wr.TEMPLATED]}
    done = {}

    def get(which):
        if which not in done:
            done[which] = _child("forms", tmp, {"P3HIP_CONV_ANY": "1"} if which == "any" else None,
                                 keys=np.array([j[0] for j in jobs[which]]), paths=np.array([j[1] for j in jobs[which]]),
                                 flags=np.array([j[2] for j in jobs[which]]))
        return done[which]
    return get


@pytest.mark.parametrize("name", wr.TEMPLATED)
def test_templated_shapes_with_the_runtime_width_1x1_kernels_bit_for_bit(forms, name):
    own, any_ = forms("own"), forms("any")
    a, b = own[name + ":wino:raw"], any_[name + ":wino:raw"]
    assert np.abs(a).max() > 0 and np.isfinite(a).all()
    assert a.tobytes() == b.tobytes(), (name, np.argwhere(a != b)[:5])
    assert str(own[name + ":wino:kernel"]) == str(any_[name + ":wino:kernel"]) == "k_wconv"


def test_the_plan_is_its_own(forms):
    """not the fp16 engine's results under another name: the raw outputs differ, by about the fp16 plan's own noise"""
    out = forms("own")
    a, b = out["test_b3c384btl3:wino:raw"], out["test_b3c384btl3:fp16:raw"]
    assert a.tobytes() != b.tobytes()
    assert 0 < np.abs(a - b).max() < 0.02
    assert str(out["test_b3c384btl3:fp16:kernel"]) == "k_lconv<3,192,192>"


@pytest.mark.parametrize("name", wr.TEMPLATED + ("test_b3c128classic", "test_b3c96nbt"))
def test_timing_hook_names_the_kernel_and_the_direct_convs_flops(forms, name):
    out = forms("own")
    w3 = wr.conv3_width(wr.config(name))                 # the file's own width, not the padded one
    assert str(out[name + ":wino:kernel"]) == "k_wconv" and float(out[name + ":wino:ms"]) > 0
    assert float(out[name + ":wino:flops"]) == 2.0 * 9 * w3 * w3 * 361 * 37


# ---- 4. composition, on one nbt net; padding ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mech(built, files, tmp_path_factory):
    return _child("mech", tmp_path_factory.mktemp("mech"), path=np.array(files(MECH_NET)),
                  pad=np.array(files("test_b3c192btl3")), garbage=np.array(files("test_b3c192btl3", garbage=True)))


def test_copies_of_a_position_and_repeated_runs_are_bit_identical(mech):
    """rows 0-31 and 96-127 of a batch of 128 hold the same positions (other units, other workgroups, other places in a
    unit: 3200 tiles apart is no multiple of 32 tiles per position); three runs on each of two engines"""
    raws = [mech["repeat:%d" % k] for k in range(6)]
    assert np.abs(raws[0]).max() > 0 and np.isfinite(raws[0]).all()
    assert raws[0][:32].tobytes() == raws[0][96:].tobytes() == raws[0][32:64].tobytes()
    assert len({r.tobytes() for r in raws}) == 1


def test_compaction_and_run_all_slots_equal_the_plain_engine(mech):
    assert np.abs(mech["plain20"]).max() > 0
    assert mech["compact"].tobytes() == mech["plain20"].tobytes()
    assert mech["allslots"].tobytes() == mech["plain20"].tobytes()


def test_launch_graph_replays_bit_for_bit(mech):
    for rnd in range(4):                       # eager, capture, replay, replay
        assert mech["graph:%d" % rnd].tobytes() == mech["graph:want"].tobytes(), rnd
    assert int(mech["graph:state"]) == 1


def test_cache_hits_equal_the_evaluation(mech):
    want = mech["plain16"][:, :362].astype(np.float32)
    assert not mech["cache:0:hit"].any() and mech["cache:1:hit"].all()
    assert mech["cache:0:logits"].tobytes() == want.tobytes() == mech["cache:1:logits"].tobytes()


def test_aux_on_top_keeps_every_other_outputs_bits(mech):
    assert mech["aux:raw"].tobytes() == mech["plain16"].tobytes()
    assert mech["aux:rec"].tobytes() == mech["plain16:rec"].tobytes()
    assert np.isfinite(mech["aux:aux"]).all() and np.abs(mech["aux:aux"]).max() > 0


def test_poisoned_scratch_changes_no_bit(mech):
    """p3hip_debug_poison with 0xFF and 0x7B in front of a full and a five-row run: the clean engine's bits (k_wconv reads
    nothing a pass did not write: off-board points and the tiles past the last are zeros made in registers)"""
    for n in (16, 5):
        clean = mech["poison:clean:%d" % n]
        assert np.isfinite(clean).all() and np.abs(clean).max() > 0
        assert clean.tobytes() == mech["plain16"][:n].tobytes()
        for mode in ("ff", "7b"):
            assert mech["poison:%s:%d" % (mode, n)].tobytes() == clean.tobytes(), (mode, n)


def test_garbage_in_the_padded_weight_channels_changes_no_bit(mech):
    """test_b3c192btl3 (C_b 96 -> 128 at load) and its zero-padded twin with garbage in the padded channels"""
    assert np.abs(mech["twin:pad"]).max() > 0
    assert mech["twin:pad"].tobytes() == mech["twin:garbage"].tobytes()
