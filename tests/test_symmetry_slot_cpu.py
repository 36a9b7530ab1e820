"""A symmetry set per slot without a GPU (P3HIP_FLAG_SYMMETRY_SLOT): the row table the engine
uploads (p3hip_debug_symmetry_rows is the function the engine calls) against a numpy cumulative sum, and the refusals
of p3hip_create_rows, which come before the weight file and the device are touched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

POP = np.array([bin(v).count("1") for v in range(256)], np.int64)


def _want(masks):
    k = POP[np.asarray(masks, np.int64)]
    return np.concatenate([[0], np.cumsum(k)[:-1]]).astype(np.int32), int(k.sum())


@pytest.mark.parametrize("n", [1, 37, 8192])
def test_row_table_equals_the_cumulative_popcounts(built, n):
    from p3achygo_amd import engine
    rng = np.random.default_rng(n)
    masks = rng.integers(1, 256, n).astype(np.uint8)
    first, total = engine.debug_symmetry_rows(masks, 8 * n)
    want_first, want_total = _want(masks)
    assert total == want_total and np.array_equal(first, want_first)
    # exactly enough rows pass, one fewer is refused
    assert engine.debug_symmetry_rows(masks, want_total)[1] == want_total
    with pytest.raises(engine.EngineError):
        engine.debug_symmetry_rows(masks, want_total - 1)


@pytest.mark.parametrize("n", [1, 37, 8192])
def test_row_table_all_eight(built, n):
    from p3achygo_amd import engine
    first, total = engine.debug_symmetry_rows(np.full(n, 0xFF, np.uint8), 8 * n)
    assert total == 8 * n and np.array_equal(first, 8 * np.arange(n))


def test_row_table_refusals(built):
    from p3achygo_amd import engine
    L = engine.lib()
    first, total = (C.c_int * 8)(), C.c_int(-1)
    masks = np.array([0xFF, 0x01, 0x10, 0x81], np.uint8)       # 8 + 1 + 1 + 2 = 12 copies
    assert L.p3hip_debug_symmetry_rows(masks.ctypes.data, 4, 12, first, C.byref(total)) == 0 and total.value == 12
    assert list(first[:4]) == [0, 8, 9, 10]
    assert L.p3hip_debug_symmetry_rows(masks.ctypes.data, 4, 11, first, C.byref(total)) == 1      # rows + 1 copies
    assert total.value == 12                                                                       # the sum is reported
    zero = np.array([0x01, 0x00, 0x03], np.uint8)
    assert L.p3hip_debug_symmetry_rows(zero.ctypes.data, 3, 24, first, C.byref(total)) == 1
    assert L.p3hip_debug_symmetry_rows(masks.ctypes.data, 0, 24, first, C.byref(total)) == 1
    assert L.p3hip_debug_symmetry_rows(masks.ctypes.data, -3, 24, first, C.byref(total)) == 1


def _refused(path, batch, flags, rows):
    from p3achygo_amd import engine
    L = engine.lib()
    assert not L.p3hip_create_rows(path.encode(), batch, 1, 0, flags, rows)
    return L.p3hip_create_error().decode()


def test_create_refusals(built, weight_files):
    from p3achygo_amd import engine
    path = weight_files("test_b3c256btl1")
    S = engine.FLAG_SYMMETRY_SLOT
    assert S == 16384
    # the plan itself is the plain engine's, whatever the other flags
    assert engine.debug_plan(path, S)[0] == engine.debug_plan(path, 0)[0]
    msg = _refused(path, 8, S | engine.FLAG_SYMMETRY_AVG, 0)
    assert "P3HIP_FLAG_SYMMETRY_SLOT" in msg and "P3HIP_FLAG_SYMMETRY_AVG" in msg
    msg = _refused(path, 8, S | engine.FLAG_AUX, 0)
    assert "P3HIP_FLAG_AUX" in msg and "P3HIP_FLAG_SYMMETRY_SLOT" in msg and "average" in msg
    for rows in (7, 65, -1):                                  # below batch, above 8 x batch
        msg = _refused(path, 8, S, rows)
        assert "symmetry_rows" in msg and str(rows) in msg and "8" in msg and "64" in msg, msg
    msg = _refused(path, 8, 0, 8)                             # rows without the flag
    assert "symmetry_rows 8" in msg and "without P3HIP_FLAG_SYMMETRY_SLOT" in msg
    msg = _refused(path, 8, engine.FLAG_SYMMETRY_AVG, 64)
    assert "without P3HIP_FLAG_SYMMETRY_SLOT" in msg
    msg = _refused(path, 16384, S, 65537)                     # above the row limit
    assert "65536" in msg
    msg = _refused(path, 16384, S, 0)                         # 0 = 8 x batch, above it as well
    assert "65536" in msg and "131072" in msg
    # in range: the refusal, if any, is no longer about the rows (without a device: the missing device)
    L = engine.lib()
    for rows in (0, 8, 15, 64):
        h = L.p3hip_create_rows(path.encode(), 8, 1, 0, S, rows)
        if h:
            L.p3hip_destroy(h)
        else:
            assert "symmetry_rows" not in L.p3hip_create_error().decode()


@pytest.mark.parametrize("keyed", [0, 1])
def test_nn_interface_device_symmetry_equals_host_rotation(built, keyed):
    """NNInterface with device symmetry over an evaluator that applies the slot's mask itself, against NNInterface with
    host rotation over the same evaluator, same positions, same PRNG: every result identical and the game's own stones,
    all eight symmetries drawn and handed over, features loaded under the identity only."""
    from p3achygo_amd import host_api
    L = host_api.lib()
    L.p3host_test_nn_device_symmetry.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_long)]
    out = (C.c_long * 9)()
    assert L.p3host_test_nn_device_symmetry(24, 4, 11, keyed, out) == 0
    differ, bad, masks, loaded_syms, mask_calls, dev_evals, host_evals, bad_root, full_masks = list(out)
    # a last pass of root visits under SetRootSymmetryMask(0xFF): every one handed over as 0xFF, results still the stones
    assert bad_root == 0 and full_masks == 24
    assert differ == 0 and bad == 0
    assert masks == 0xFF                     # every one of the eight went to the engine as a one-bit mask
    assert loaded_syms == 0x01               # the features always under the identity
    assert mask_calls == 24 * 4              # one mask per evaluation that reached the engine
    assert dev_evals == host_evals == (24 if keyed else 24 * 4)


def test_selfplay_device_symmetry_needs_the_engine_symbols(built, weight_files):
    """the CPU engine under oracle/ has no p3hip_create_rows: a self-play run that asks for device symmetry fails with
    a message; without the option the same run works"""
    from conftest import ROOT
    from p3achygo_amd import host_api
    lib = os.path.join(ROOT, "oracle", "libp3cpu_engine.so")
    os.environ["P3CPU_THREADS"] = "2"
    w = weight_files("test_b3c128btl2")
    kw = dict(num_games=4, num_threads=1, seconds=0.0, default_n=4, default_k=2, selected_n=4, selected_k=2,
              max_moves=6, warmup_batches=0, seed=3, engine_lib=lib)
    host_api.set_groups(1)
    host_api.set_step_limit(2)
    try:
        host_api.set_device_symmetry(1)
        with pytest.raises(RuntimeError, match="p3hip_create_rows"):
            host_api.selfplay_run(w, **kw)
        host_api.set_device_symmetry(0)
        assert host_api.selfplay_run(w, **kw).batches == 2
    finally:
        host_api.set_device_symmetry(0)
        host_api.set_step_limit(0)
        host_api.set_groups(2)


def test_eval_player_keys_parse(built, tmp_path):
    from p3achygo_amd import host_api
    L = host_api.lib()
    L.p3host_parse_player_device_symmetry.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.c_char_p]
    p = tmp_path / "player.cfg"
    dev, mask, err = C.c_int(7), C.c_uint32(7), C.create_string_buffer(256)

    def parse(text):
        p.write_text(text)
        return L.p3host_parse_player_device_symmetry(str(p).encode(), C.byref(dev), C.byref(mask), err)

    assert parse("n: 16\n") == 0 and (dev.value, mask.value) == (0, 0)
    assert parse("nn_device_symmetry: 1\n") == 0 and (dev.value, mask.value) == (1, 0)
    assert parse("nn_device_symmetry: 0\n") == 0 and (dev.value, mask.value) == (0, 0)
    for text, want in (("255", 255), ("0xFF", 255), ("0x81", 0x81), ("129", 129), ("1", 1)):
        assert parse(f"n: 16\nnn_root_symmetry_mask: {text}\n") == 0, (text, err.value)
        assert (dev.value, mask.value) == (1, want), text          # the key implies device symmetry
    assert parse("nn_root_symmetry_mask: 0\n") == 0 and (dev.value, mask.value) == (0, 0)   # 0 = off
    assert parse("nn_device_symmetry: 1\nnn_root_symmetry_mask: 0\n") == 0 and (dev.value, mask.value) == (1, 0)
    for text in ("256", "0x100", "-1", "ten", "0x", "1.5"):
        assert parse(f"nn_root_symmetry_mask: {text}\n") == 1, text
        assert b"nn_root_symmetry_mask" in err.value
    for text in ("2", "yes", "-1", "0x1"):
        assert parse(f"nn_device_symmetry: {text}\n") == 1, text
        assert b"nn_device_symmetry" in err.value


def test_eval_match_device_symmetry_needs_the_engine_symbols(built, weight_files):
    """the CPU engine under oracle/ has no p3hip_create_rows: a match whose player asks for device symmetry or a root
    mask fails with a message on both eval paths, and so does the root mask together with nn_symmetry_mask; over the
    null evaluator the keys are accepted and the match plays"""
    from conftest import ROOT
    from p3achygo_amd import host_api
    lib = os.path.join(ROOT, "oracle", "libp3cpu_engine.so")
    w = weight_files("test_b3c128btl2")
    os.environ["P3CPU_THREADS"] = "2"
    try:
        for text in ("nn_device_symmetry: 1\n", "nn_root_symmetry_mask: 0xff\n"):
            host_api.eval_set_player_flags(cand=text)
            with pytest.raises(RuntimeError, match="p3hip_create_rows"):
                host_api.eval_match_threads(w, w, num_games=2, visits_per_move=4, threads_per_game=2, max_moves=4,
                                            seed=3, engine_lib=lib)
            with pytest.raises(RuntimeError, match="p3hip_create_rows"):
                host_api.eval_match(w, w, num_games=2, visits_per_move=4, leaves_per_round=2, max_moves=4,
                                    num_threads=1, seed=3, engine_lib=lib)
        host_api.eval_set_player_flags(cand="nn_root_symmetry_mask: 0xff\nnn_symmetry_mask: 0x0f\n")
        with pytest.raises(RuntimeError, match="nn_symmetry_mask cannot be combined"):
            host_api.eval_match(w, w, num_games=2, visits_per_move=4, leaves_per_round=2, max_moves=4, num_threads=1,
                                seed=3, engine_lib=lib)
        host_api.eval_set_player_flags(cand="nn_root_symmetry_mask: 0xff\n")
        st = host_api.eval_match(None, None, num_games=2, visits_per_move=8, leaves_per_round=2, max_moves=6,
                                 num_threads=1, seed=3)
        assert st.games == 2
    finally:
        host_api.eval_set_player_flags()
