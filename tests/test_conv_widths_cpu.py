"""Conv trunks of any width from 64 to 512 channels without a GPU: the set's definition (netspec.conv_supported,
P3HIP_CONV_SET), p3hip_create's architecture check, which packs, pads and plans before it looks for a device, the
table netspec.WIDE_CONV_CONFIGS, the fp16 emulation against the bounds of tests/test_conv_widths_gpu.py, the twin of
the block-by-block nets against trunk_emulation's layer-wise bounds, the importer, and the register / LDS budget of
the kernels of csrc/conv_any.hip read from the compiler's assembly."""
import dataclasses
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import conv_widths_common as cw  # noqa: E402
import trunk_emulation as te  # noqa: E402

H5 = os.path.join(ROOT, "tests", "golden", "h5")
CSRC = os.path.join(ROOT, "p3achygo_amd", "csrc")


def _cfg(C, Cb, kind="btl", inner=2, H=32, V=64, interval=3, blocks=3):
    from p3achygo_amd import netspec
    return netspec.NetConfig("probe", blocks, C, Cb, H, V, interval, inner, kind)


def test_conv_supported_on_a_grid_of_shapes():
    from p3achygo_amd import netspec
    ok = netspec.conv_supported
    for C in range(16, 640, 16):
        for Cb in range(16, 640, 16):
            want = C % 32 == 0 and 64 <= C <= 512 and Cb % 16 == 0 and 32 <= Cb <= C
            for kind, inner in (("btl", 1), ("btl", 3), ("nbt", 2)):
                assert ok(_cfg(C, Cb, kind, inner)) == want, (C, Cb, kind)
            assert ok(_cfg(C, Cb, "classic", 2)) == (C % 32 == 0 and 64 <= C <= 512), (C, Cb)
    assert not ok(_cfg(128, 64, "btl", 4)) and not ok(_cfg(128, 64, "btl", 0)) and not ok(_cfg(128, 64, "classic", 3))
    assert not ok(_cfg(128, 64, H=16)) and not ok(_cfg(128, 64, V=40)) and all(ok(_cfg(128, 64, V=v)) for v in (32, 48, 64, 80))
    assert not ok(_cfg(128, 64, interval=1)) and ok(_cfg(128, 64, interval=2)) and ok(_cfg(128, 64, interval=9))
    assert not ok(netspec.CONFIGS["tiny"]) and not ok(netspec.TRANSFORMER_CONFIGS["test_b2d96h3_tfm"])
    # every conv net the engine ran before is in the set, and every net of the new table
    assert all(ok(c) for n, c in netspec.CONFIGS.items() if n != "tiny")
    assert all(ok(c) for c in netspec.WIDE_CONV_CONFIGS.values())


def test_conv_set_is_stated_once_in_the_header_and_repeated_in_netspec():
    from p3achygo_amd import netspec
    hdr = open(os.path.join(ROOT, "include", "p3hip.h")).read()
    assert hdr.count("#define P3HIP_CONV_SET") == 1
    m = re.search(r"#define P3HIP_CONV_SET \\\n((?:\s*\"[^\n]*\"(?: \\)?\n)+)", hdr)
    assert m, "P3HIP_CONV_SET is not a string macro"
    assert "".join(re.findall(r"\"([^\"]*)\"", m.group(1))) == netspec.CONV_SET


def test_wide_conv_table_is_apart_and_covers_the_ground():
    from p3achygo_amd import netspec
    T = netspec.WIDE_CONV_CONFIGS
    assert set(cw.NETS) <= set(T)
    assert not set(T) & (set(netspec.CONFIGS) | set(netspec.TRANSFORMER_CONFIGS) | set(netspec.WIDE_TRANSFORMER_CONFIGS))
    assert all(netspec.get_config(n) is c for n, c in T.items())
    cfgs = [T[n] for n in cw.NETS]
    assert {c.block_type for c in cfgs} == {"btl", "nbt", "classic"}
    assert {c.c_val for c in cfgs} == {32, 48, 64, 80}
    assert {c.channels for c in cfgs} >= {64, 512} and any(c.channels % 64 for c in cfgs)
    assert any(c.bottleneck_channels % 64 for c in cfgs) and any(2 * c.bottleneck_channels < c.channels for c in cfgs)


def _create(path, flags=0):
    """p3hip_create on device 0: (engine handle or None, error message)"""
    from p3achygo_amd import engine
    L = engine.lib()
    h = L.p3hip_create(path.encode(), 4, 1, 0, flags)
    return h, (L.p3hip_create_error() or b"").decode()


def _write(tmp_path, cfg, randomize=False):
    from p3achygo_amd import netspec
    path = str(tmp_path / (cfg.name + ".p3w"))
    netspec.save_p3w(path, cfg, netspec.generate_weights(cfg, randomize=randomize))
    return path


@pytest.mark.parametrize("name", cw.NETS + ["b14c320btl3"])
def test_create_accepts_every_net_of_the_table(built, tmp_path, name):
    """packing, padding and the plan are accepted before the device is looked for: without a GPU the only refusal is
    the missing device"""
    from p3achygo_amd import engine, netspec
    h, err = _create(_write(tmp_path, netspec.WIDE_CONV_CONFIGS[name]))
    if h:
        engine.lib().p3hip_destroy(h)
    else:
        assert err.startswith("no HIP device"), err


@pytest.mark.parametrize("cfg", [
    _cfg(48, 32), _cfg(544, 256), _cfg(200, 96), _cfg(128, 160), _cfg(128, 64, "btl", 4), _cfg(128, 64, H=16),
    _cfg(128, 64, V=40), _cfg(96, 24, "nbt"), _cfg(544, 64, "classic")], ids=lambda c: f"C{c.channels}_Cb{c.bottleneck_channels}_{c.block_type}{c.inner_layers}_H{c.head_channels}_V{c.c_val}")
def test_create_refuses_shapes_outside_the_set_by_name(built, tmp_path, cfg):
    from p3achygo_amd import netspec
    assert not netspec.conv_supported(cfg)
    h, err = _create(_write(tmp_path, cfg))
    assert not h
    assert err.startswith("unsupported architecture") and netspec.CONV_SET in err and netspec.TRANSFORMER_SET in err, err


def test_create_still_refuses_tiny(built, tmp_path):
    from p3achygo_amd import netspec
    h, err = _create(_write(tmp_path, netspec.CONFIGS["tiny"]))
    assert not h and err.startswith("unsupported architecture") and netspec.CONV_SET in err, err


@pytest.mark.parametrize("name", ["test_b3c192btl3", "test_b3c512nbt", "test_b3c128classic", "test_b3c256btl2_cb64"])
def test_create_refuses_int8_on_a_new_shape(built, tmp_path, name):
    """either INT8 flag: refused with the shapes INT8 serves"""
    from p3achygo_amd import engine, netspec
    path = _write(tmp_path, netspec.WIDE_CONV_CONFIGS[name])
    for flag in (engine.FLAG_INT8, engine.FLAG_INT8_FUSED):
        h, err = _create(path, flag)
        assert not h
        assert "INT8" in err and "C = 384 / C_b = 192" in err and "C = 256 / C_b = 128" in err and "C = 192 classic" in err, err


def test_p3w_round_trip_and_flops_of_the_table(tmp_path):
    from p3achygo_amd import netspec
    L = 361
    for name, cfg in netspec.WIDE_CONV_CONFIGS.items():
        if cfg.blocks > 4:
            continue
        W = netspec.generate_weights(cfg, randomize=True)
        p = str(tmp_path / (name + ".p3w"))
        netspec.save_p3w(p, cfg, W)
        c2, W2, _ = netspec.load_p3w(p)
        assert dataclasses.replace(c2, name=name) == cfg
        assert set(W2) == set(W) and all(np.array_equal(W2[k], W[k]) for k in W)
    for name, cfg in netspec.WIDE_CONV_CONFIGS.items():
        C, Cb, H = cfg.channels, cfg.bottleneck_channels, cfg.head_channels
        nb = sum(cfg.block_kind(i) == "broadcast" for i in range(cfg.blocks))
        n3 = {"btl": cfg.inner_layers, "nbt": 4, "classic": 2}[cfg.block_type]
        w3 = C if cfg.block_type == "classic" else Cb
        conv3 = 2.0 * (cfg.blocks - nb) * L * n3 * 9 * w3 * w3
        total, c3 = netspec.flops_per_position(cfg)
        assert abs(c3 - conv3) < 1.0, name
        one = 0.0 if cfg.block_type == "classic" else 2.0 * (cfg.blocks - nb) * L * 2 * C * Cb
        bc = 2.0 * nb * (L * 2 * C * C + C * L * L)
        stem_heads = netspec.flops_per_position(dataclasses.replace(cfg, blocks=0))[0]
        assert abs(total - (conv3 + one + bc + stem_heads)) < 1.0, name


@pytest.mark.parametrize("name", cw.PADDED_NETS + ["test_b3c64btl2"])
def test_zero_padding_rule_changes_no_output_and_keeps_padded_channels_zero(name):
    """the rule the engine pads by, restated in numpy (conv_widths_common.pad_weights) and run through the float64
    restatement and the fp16 emulation: padded channels of x are exactly 0 after every block (the folded BN of a padded
    channel is scale = shift = 0, mish(0) = 0; the broadcast dense's bias is removed by the zero bn1), the others and
    every output are what the unpadded net gives"""
    cfg, W = cw.config(name), cw.weights(name)
    big, Wp = cw.pad_weights(cfg, W)
    assert (big.channels, big.bottleneck_channels) != (cfg.channels, cfg.bottleneck_channels)
    assert big.channels % 64 == 0 and big.bottleneck_channels % 64 == 0
    pos = cw.positions(4)
    for fp16 in (False, True):
        xs = cw.trunk(cfg, W, fp16=fp16).trunk(features=pos)
        xp = cw.trunk(big, Wp, fp16=fp16).trunk(features=pos)
        for a, b in zip(xs, xp):
            assert (b[:, cfg.channels:] == 0).all()
            assert np.abs(a.numpy() - b[:, :cfg.channels].numpy()).max() <= 1e-9
        a, b = cw.outputs(cfg, W, pos, fp16), cw.outputs(big, Wp, pos, fp16)
        assert all(np.abs(a[k] - b[k]).max() <= 1e-9 for k in a)


@pytest.fixture(scope="module")
def emulated():
    """name -> the six error columns of the fp16 emulation against the float64 restatement, 16 positions (seed 11)"""
    pos = cw.positions()
    out = {}
    for name in cw.NETS:
        cfg, W = cw.config(name), cw.weights(name)
        out[name] = cw.emulated_errors(cw.outputs(cfg, W, pos, False), cw.outputs(cfg, W, pos, True))
        print(name, {k: float("%.3g" % v) for k, v in out[name].items()})
    return out


def test_fp16_emulation_stays_inside_half_the_gpu_bounds(emulated):
    """every bound of tests/test_conv_widths_gpu.py is at least twice what the emulation measures, and the table the
    bounds were derived from still holds (each entry rounds the measurement up by at most a tenth)"""
    from test_conv_widths_gpu import EMULATED, TOL
    assert set(TOL) == set(emulated) == set(cw.NETS)
    for name, e in emulated.items():
        t = TOL[name]
        assert e["logit"] <= t["logit"] / 2 or e["logit_share"] <= 0.5, (name, e)
        assert (t["logit"] == cw.LOGIT_TOL) == (e["logit_share"] <= 0.5), (name, e)
        for c in cw.COLUMNS[1:]:
            assert e[c] <= t[c] / 2, (name, c, e[c], t[c])
            assert t[c] >= cw.BASE[c]
        for c, v in EMULATED[name].items():
            assert e[c] <= v <= 1.1 * e[c] + 1e-12, (name, c, e[c], v)


def test_twin_of_the_block_nets_is_inside_half_the_layerwise_bounds():
    """The twin (engine storage points, other fp32 arithmetic) in place of the engine on the 37-position batch of
    test_blocks_teacher_forced: trunk_emulation's layer-wise bounds were set from widths up to 384, so a net keeps a
    bound only where its twin's worst error is at most half of it and its identical fraction at least the bound's."""
    from test_conv_widths_gpu import BLOCK_BOUNDS, block_batch
    pos, slots = block_batch(37)
    for name in cw.BLOCK_NETS:
        cfg, W = cw.config(name), cw.weights(name)
        xt = cw.trunk(cfg, W, twin=True).trunk(pos[slots])
        st = cw.teacher_forced(cw.trunk(cfg, W), xt, pos[slots], slots=slots, label=name + " block ",
                               bounds=BLOCK_BOUNDS[name])
        print(name, {k: (round(v["max_err"], 2), round(v["identical"], 3)) for k, v in st.items()})
        for k, v in st.items():
            key = "stem" if k == "stem" else cw.kind_of(cfg, k)
            max_err, min_identical = BLOCK_BOUNDS[name].get(key, te.BOUNDS[key])
            assert v["max_err"] <= max_err / 2 and v["identical"] >= min_identical, (name, k, key, v["max_err"], v["identical"])


def _constructor_arguments(cfg):
    """the P3achyGoModel constructor arguments of a conv net (model.py:1128-1150)"""
    return dict(name=cfg.name, num_blocks=cfg.blocks, num_channels=cfg.channels,
                num_bottleneck_channels=cfg.bottleneck_channels, num_head_channels=cfg.head_channels, c_val=cfg.c_val,
                broadcast_interval=cfg.broadcast_interval, trunk_block_type=cfg.block_type,
                bottleneck_length=cfg.inner_layers + 2)


@pytest.mark.parametrize("name", ["test_b3c96nbt", "test_b3c192btl3", "test_b3c128classic"])
def test_keras_import_of_a_synthetic_archive_of_a_new_shape(built, tmp_path, name, capsys):
    from p3achygo_amd import engine, keras_import, keras_map, netspec
    cfg = netspec.WIDE_CONV_CONFIGS[name]
    assert keras_import.config_from_arguments(_constructor_arguments(cfg)) == cfg
    other = dataclasses.replace(cfg, name="other", blocks=cfg.blocks + 1)   # a shape of no table keeps its fields
    got = keras_import.config_from_arguments(_constructor_arguments(other))
    assert dataclasses.replace(got, name="other") == other
    W = netspec.generate_weights(cfg, randomize=True)
    datasets = {path: W[tensor] for path, tensor in keras_map.object_path_map(cfg)}
    datasets["optimizer/vars/0"] = np.zeros(3, np.float32)
    tensors, unused = keras_import.convert(datasets, cfg)
    assert unused == ["optimizer/vars/0"]
    assert set(tensors) == set(W) and all(tensors[k].tobytes() == W[k].tobytes() for k in W)
    path = str(tmp_path / "imported.p3w")
    netspec.save_p3w(path, cfg, tensors)
    _, W2, _ = netspec.load_p3w(path)
    assert all(W2[k].tobytes() == W[k].tobytes() for k in W)
    h, err = _create(path)
    if h:
        engine.lib().p3hip_destroy(h)
    else:
        assert err.startswith("no HIP device"), err


def test_keras_import_notes_a_conv_checkpoint_the_engine_will_not_run(tmp_path, capsys):
    """tiny (C = 16, H = 8) is converted as before, with status 0, and one line on stderr quotes the set"""
    from p3achygo_amd import keras_import, netspec
    dst = str(tmp_path / "tiny.p3w")
    assert keras_import.main([os.path.join(H5, "tiny_p3achygo.keras"), dst]) == 0
    cap = capsys.readouterr()
    note = [l for l in cap.err.splitlines() if l.strip()]
    assert len(note) == 1 and "will not run" in note[0] and netspec.CONV_SET in note[0], cap.err
    assert netspec.load_p3w(dst)[0].channels == 16


def test_keras_import_of_a_shape_inside_the_set_is_silent(tmp_path, capsys, monkeypatch):
    from p3achygo_amd import keras_import, keras_map, netspec
    cfg = netspec.WIDE_CONV_CONFIGS["test_b3c64btl2"]
    W = netspec.generate_weights(cfg)
    datasets = {path: W[tensor] for path, tensor in keras_map.object_path_map(cfg)}
    config = {"class_name": "P3achyGoModel", "config": _constructor_arguments(cfg)}
    monkeypatch.setattr(keras_import, "read_archive", lambda path: (datasets, config))
    got, _ = keras_import.import_checkpoint("synthetic.keras", str(tmp_path / "a.p3w"))
    assert got == cfg and capsys.readouterr().err == ""


# ---- kernel resources (the manner of tests/test_kernel_resources_cpu.py) ------------------------------------------

def _assembly():
    import shutil
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    h = hashlib.sha256()
    for f in ("conv_any.hip", "conv_any.h", "kernels.h", "conv_core.h", "layer_kernels.h", "launch_util.h",
              "stem_planes.inc", "stem_epilogue.inc", "bdense_epilogue.inc", "bdense_transpose.inc"):
        h.update(open(os.path.join(CSRC, f), "rb").read())
    out = os.path.join(ROOT, "build", "conv_any_gfx950_%s.s" % h.hexdigest()[:16])
    if not os.path.exists(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        for old in os.listdir(os.path.dirname(out)):
            if old.startswith("conv_any_gfx950_") and old.endswith(".s"):
                os.remove(os.path.join(os.path.dirname(out), old))
        r = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                            os.path.join(CSRC, "conv_any.hip"), "-o", out + ".tmp"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + ".tmp", out)
    return open(out).read()


def _geo_act_bytes(npos, cb, kw):
    """conv_core.h Geo<NPOS, CB, KW>::ACT_BYTES"""
    pad = kw // 2
    s = 19 + pad
    nrows, padtop = 18 * s + 19, pad * s + pad
    return (npos * (padtop + nrows + padtop) * (cb * 2 + 16) + 15) // 16 * 16


def _ring_bytes(cout_pass, kms=4, depth=2):
    return (depth + 1) * kms * cout_pass * 32


def test_runtime_width_kernels_use_no_scratch_and_fit_their_lds_and_registers():
    """every kernel of conv_any.hip: no scratch, no static LDS beside the dynamic allocation, and the dynamic LDS its
    launcher asks for (restated from conv_any.hip) within 160 KiB per CU, or 80 KiB where two workgroups share one;
    the registers of the 4-wave layer conv leave room for the second workgroup (two waves per SIMD: 256 VGPRs each)"""
    asm = _assembly()
    kernels = {}
    for m in re.finditer(r"^(_ZN2p3\d+(k_\w+?_any)\w*):\s", asm, re.M):
        body = asm[m.start():asm.index(".Lfunc_end", m.start())]
        meta = asm[asm.index(".Lfunc_end", m.start()):]
        get = lambda key: int(re.search(r"; %s: (\d+)" % key, meta).group(1))
        kernels[m.group(1)] = dict(kind=m.group(2), scratch_ops=body.count("scratch_"), scratch=get("ScratchSize"),
                                   vgprs=get("NumVgprs") + get("NumAgprs"), lds=get("LDSByteSize"))
    kinds = [k["kind"] for k in kernels.values()]
    assert kinds.count("k_lconv_any") == 10 and kinds.count("k_conv1x1_any") == 6 and kinds.count("k_init_any") == 2 \
        and kinds.count("k_bdense_any") == 1, sorted(kernels)
    for name, k in kernels.items():
        assert k["scratch"] == 0 and k["scratch_ops"] == 0, (name, k)
        assert k["lds"] == 0, (name, k)
        assert k["vgprs"] <= (256 if k["kind"] == "k_lconv_any" else 512), (name, k)
    KiB = 1024
    for kw in (1, 3):   # k_lconv_any: Geo<1, 64, KW, 4, KW == 3 ? 2 : 4>, two workgroups per CU
        assert 2 * (_geo_act_bytes(1, 64, kw) + _ring_bytes(64, 2 if kw == 3 else 4)) <= 160 * KiB
    for cp in (64, 128):   # k_init_any: Geo<1, 16, 5>, the ring and one bias float per channel, two per CU
        assert 2 * (_geo_act_bytes(1, 16, 5) + _ring_bytes(cp) + 512 * 4) <= 160 * KiB
    for cb, cp in ((64, 64), (128, 128), (128, 64)):   # k_conv1x1_any: Geo<128 / CB, CB, 1>
        assert _geo_act_bytes(128 // cb, cb, 1) + _ring_bytes(cp) <= 160 * KiB
    # k_bdense_any: Tt (128 channel rows of 784 bytes), the ring of 128-column passes, bias [384] + bn1 [2][512]
    assert 128 * 784 + _ring_bytes(128) + (384 + 2 * 512) * 4 <= 160 * KiB
