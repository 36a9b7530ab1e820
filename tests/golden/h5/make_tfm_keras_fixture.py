"""Writes tests/golden/h5/tfm_b2d64h2_p3achygo.keras and its tensor hashes: a transformer checkpoint (a generic_arch of two
["transformer", {"embed_dim": 64, "num_heads": 2}] blocks, netspec's test_b2d64h2_tfm) in the Keras 3 object-path
layout keras_map.object_path_map describes, weights from netspec.generate_weights (randomize=True), plus an optimizer
variable a real checkpoint also carries.  Written FROM the map, with the HDF5 library: it pins the importer's plumbing
for transformer trunks (config.json's generic_arch, paths, shapes), not Keras's naming.  config.json holds what
P3achyGoModel.get_config returns (model.py:1572-1590) after construct_trunk_from_generic_arch has added pos_len and
name to every block entry (model.py:1054), and ModelConfig's default num_blocks 16 (model_config.py:34, :166-172).

Run with an interpreter that has h5py (the one tests/golden/h5/make_h5_fixtures.py names):
    /opt/conda/bin/python3.9 tests/golden/h5/make_tfm_keras_fixture.py
"""
import hashlib
import io
import json
import os
import sys
import zipfile

import h5py
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.normpath(os.path.join(HERE, "..", "..", "..")))
from p3achygo_amd import keras_map, netspec   # numpy only

cfg = netspec.WIDE_TRANSFORMER_CONFIGS["test_b2d64h2_tfm"]
W = netspec.generate_weights(cfg, randomize=True)
buf = io.BytesIO()
with h5py.File(buf, "w") as f:
    for path, name in keras_map.object_path_map(cfg):
        f.create_dataset(path, data=W[name].astype(np.float32))
    f.create_dataset("optimizer/vars/0", data=np.int64(1234))
trunk = [["transformer", {"embed_dim": cfg.channels, "num_heads": cfg.bottleneck_channels, "pos_len": 19,
                          "name": f"transformer_{i}"}] for i in range(cfg.blocks)]
config = {"module": "model", "class_name": "P3achyGoModel", "registered_name": "p3achygo>P3achyGoModel",
          "config": {"board_len": 19, "num_input_planes": 15, "num_input_features": 8, "num_blocks": 16,
                     "num_channels": cfg.channels, "num_bottleneck_channels": 64, "num_head_channels": cfg.head_channels,
                     "c_val": cfg.c_val, "bottleneck_length": 4, "conv_size": 3, "broadcast_interval": 8,
                     "trunk_block_type": "btl", "generic_arch": {"trunk": trunk}, "is_transformer": True, "c_l2": 0.0,
                     "name": "p3achygo"}}
with zipfile.ZipFile(os.path.join(HERE, "tfm_b2d64h2_p3achygo.keras"), "w", zipfile.ZIP_DEFLATED) as z:
    z.writestr("metadata.json", json.dumps({"keras_version": "3.3.3"}))
    z.writestr("config.json", json.dumps(config))
    z.writestr("model.weights.h5", buf.getvalue())
with open(os.path.join(HERE, "tfm_b2d64h2_p3achygo_sha256.json"), "w") as f:
    json.dump({n: [list(W[n].shape), hashlib.sha256(np.ascontiguousarray(W[n], np.float32).tobytes()).hexdigest()]
               for n in sorted(W)}, f, indent=0)
print("tfm_b2d64h2_p3achygo.keras", os.path.getsize(os.path.join(HERE, "tfm_b2d64h2_p3achygo.keras")), "bytes")
