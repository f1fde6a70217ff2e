"""The ternary checkpoints of the reference (results/RESNET3/weights_{tf,tt}.hdf5, converted by
tools/import_keras_hdf5.py and re-packed by tools/pack_keras_npz.py) load through nets.spec_from_keras_npz and
run on the oracle; the LeakyReLU epilogue constant of the C ABI (include/qnn_abi.h) and its Python mirror."""
import json
import os
import re

import numpy as np
import pytest

from qnn_amd import _abi, nets
from oracle import qnn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("code", ["tf", "tt"])
def test_ternary_checkpoint_spec(code):
    path = os.path.join(GOLD, "resnet3_full_%s.npz" % code)
    spec = nets.spec_from_keras_npz(path, 4, 4)
    d = np.load(path)
    layers = {l["name"]: l["config"] for l in json.loads(bytes(d["model_config_json"]).decode())["config"]["layers"]}
    convs = [op for op in spec if op["op"] == "conv"]
    dense = [op for op in spec if op["op"] == "dense"]
    assert len(convs) == 21 and all(op["kind"] == "ternary" for op in convs)
    assert len(dense) == 1 and dense[0]["kind"] == "ternary"
    for op in convs + dense:
        cfg = layers[op["dst"]]
        assert op["H"] == float(cfg["H"])
        assert op["klm"] == np.float32(cfg["kernel_lr_multiplier"])
        assert (op["bias"] is not None) == bool(cfg["use_bias"])
        np.testing.assert_array_equal(op["kernel"], d[op["dst"] + "/kernel"])
    assert spec[-1]["op"] == "softmax"
    acts = [op["fn"] for op in spec if op["op"] == "act"]
    assert set(acts) == ({"leaky_relu"} if code == "tf" else {"ternary_tanh"})
    x = nets.synthetic_images(nets.Config(dim=32), 4, 5)
    logits = O.run_spec(spec[:-1], x)
    assert logits.shape == (4, 10) and np.all(np.isfinite(logits))


def test_leaky_relu_constant():
    assert _abi.FN_LEAKY_RELU == 5
    src = open(os.path.join(ROOT, "include", "qnn_abi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    defs = dict(re.findall(r"#define\s+(QNN_FN_[A-Z_]+)\s+(\d+)", src))
    assert defs["QNN_FN_LEAKY_RELU"] == "5"
    assert len(set(defs.values())) == len(defs)          # no two activations share a code
