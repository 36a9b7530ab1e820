"""`.keras` import of transformer checkpoints (p3achygo_amd/keras_import.py, keras_map): a synthetic archive of a
generic_arch trunk written with the HDF5 library from keras_map.object_path_map (tests/golden/h5/make_tfm_keras_fixture.py)
becomes a .p3w whose tensors are the written arrays, and archives the engine cannot run are refused with the wording of
include/p3hip.h.  No archive saved by the reference's own Keras model exists here: parity with one is unpinned."""
import hashlib
import io
import json
import os
import zipfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H5 = os.path.join(ROOT, "tests", "golden", "h5")
SRC = os.path.join(H5, "tfm_b2d64h2_p3achygo.keras")


def test_transformer_archive_imports_to_the_written_tensors(tmp_path):
    from p3achygo_amd import keras_import, netspec
    dst = str(tmp_path / "t.p3w")
    assert keras_import.main([SRC, dst]) == 0
    cfg, unused = keras_import.import_checkpoint(SRC, dst)
    assert cfg == netspec.WIDE_TRANSFORMER_CONFIGS["test_b2d64h2_tfm"]
    assert unused == ["optimizer/vars/0"]
    cfg2, tensors, _ = netspec.load_p3w(dst)
    assert (cfg2.blocks, cfg2.channels, cfg2.bottleneck_channels, cfg2.block_type) == (2, 64, 2, "transformer")
    want = json.load(open(os.path.join(H5, "tfm_b2d64h2_p3achygo_sha256.json")))
    assert set(tensors) == set(want) == {n for n, _, _ in netspec.tensor_specs(cfg)}
    for name, (shape, digest) in want.items():
        a = tensors[name]
        assert list(a.shape) == shape and a.dtype == np.float32
        assert hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() == digest, name


def test_object_paths_of_transformer_blocks():
    """TransformerBlock's attributes (model_transformer.py:216-237) under the members of the `blocks` list"""
    from p3achygo_amd import keras_map, netspec
    for cfg in list(netspec.TRANSFORMER_CONFIGS.values()) + list(netspec.WIDE_TRANSFORMER_CONFIGS.values()):
        for rows in (keras_map.object_path_map(cfg), keras_map.name_map(cfg)):
            assert len({k for k, _ in rows}) == len(rows)
            assert {p for _, p in rows} == {n for n, _, _ in netspec.tensor_specs(cfg)}
    rows = dict((p, k) for k, p in keras_map.object_path_map(netspec.TRANSFORMER_CONFIGS["b14d96h3_transformer"]))
    assert rows["blocks.0.q.w"] == "blocks/transformer_block/Q/vars/0"
    assert rows["blocks.13.rms_out.scale"] == "blocks/transformer_block_13/rms_out/vars/0"
    assert rows["blocks.2.ffn_down.w"] == "blocks/transformer_block_2/ffn_down/vars/0"
    names = dict((p, k) for k, p in keras_map.name_map(netspec.TRANSFORMER_CONFIGS["b14d96h3_transformer"]))
    assert names["blocks.3.k.w"] == "transformer_3/key/kernel"
    assert names["blocks.0.ffn_gate.w"] == "transformer_0/swiglu_gate/kernel"


def _with_config(tmp_path, edit):
    """the fixture archive with its config.json edited by `edit(model arguments)`"""
    out = str(tmp_path / "edited.keras")
    with zipfile.ZipFile(SRC) as z, zipfile.ZipFile(out, "w") as w:
        for n in z.namelist():
            data = z.read(n)
            if n == "config.json":
                c = json.loads(data)
                edit(c["config"])
                data = json.dumps(c).encode()
            w.writestr(n, data)
    return out


def _trunk(blocks):
    return {"trunk": [["transformer", {"embed_dim": d, "num_heads": h}] for d, h in blocks]}


@pytest.mark.parametrize("edit,match", [
    (lambda a: a.update(generic_arch=_trunk([(64, 2), (64, 1)])), "different \\(embed_dim, num_heads\\)"),
    (lambda a: a.update(num_channels=96), "embed_dim 64 differs from the stem's num_channels 96"),
    (lambda a: a.update(generic_arch=_trunk([(64, 4), (64, 4)])), "unsupported architecture"),
    (lambda a: a.update(num_channels=416, generic_arch=_trunk([(416, 13)] * 2)), "unsupported architecture"),
    (lambda a: a.update(generic_arch={"trunk": [["conv", {}]]}), "transformer trunks only"),
])
def test_archives_the_engine_cannot_run_are_refused(tmp_path, edit, match):
    from p3achygo_amd import keras_import, netspec
    with pytest.raises(ValueError, match=match) as e:
        keras_import.import_checkpoint(_with_config(tmp_path, edit), str(tmp_path / "x.p3w"))
    assert netspec.TRANSFORMER_SET in str(e.value)
    assert not os.path.exists(tmp_path / "x.p3w")
