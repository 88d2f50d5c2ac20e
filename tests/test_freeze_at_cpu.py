"""MODEL.BACKBONE.FREEZE_AT 0 / 1 without a GPU: the argmax and summation rule of the pool backward against ATen, the stem's layout
round trip, the trainable-layer sets, the solver key and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proj_roadsurf_amd import train_model
from proj_roadsurf_amd.spec import EngineSpec
from proj_roadsurf_amd.weights import (STEM_CIN_PAD, STEM_KW_PAD, conv_layers, engine_tensors, master_to_d2, packed_tensors, synthetic_weights, train_tensors,
                                       trainable_layers)
from tests import freeze_at_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pool_inputs(kind: str, n: int, h: int, w: int, c: int, seed: int):
    """(x, dq): the pool's input after the ReLU (``ties``: drawn from {0, 0.5, 1, 2}, many equal maxima and zeros; ``continuous``: a
    normal draw through the ReLU) and a gradient of the pooled map, both fp16-representable float32."""
    rng = np.random.default_rng(seed)
    if kind == "ties":
        x = rng.choice(np.array([0.0, 0.5, 1.0, 2.0], np.float32), size=(n, h, w, c))
    else:
        x = np.maximum(rng.standard_normal((n, h, w, c)), 0).astype(np.float16).astype(np.float32)
    dq = rng.standard_normal((n, R.pooled_size(h), R.pooled_size(w), c)).astype(np.float16).astype(np.float32)
    return x, dq


@pytest.mark.parametrize("kind", ["ties", "continuous"])
@pytest.mark.parametrize("hw", [(6, 6), (8, 12), (10, 6), (7, 9)])
def test_pool_backward_restatement_equals_autograd(kind, hw):
    """relu + max_pool2d(3, 2, 1) through torch.autograd on the CPU, bit for bit: pins the argmax rule (first maximum in (row, column)
    order) and the order of the up to four additions per pixel."""
    h, w = hw
    x, dq = pool_inputs(kind, 2, h, w, 8, seed=h * 100 + w)
    # a pre-ReLU tensor whose ReLU is x: negative where x is zero
    pre = torch.from_numpy(np.where(x > 0, x, -1.0).astype(np.float32)).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.max_pool2d(F.relu(pre), 3, 2, 1)
    y.backward(torch.from_numpy(dq).permute(0, 3, 1, 2).contiguous())
    want = pre.grad.permute(0, 2, 3, 1).numpy()
    got = R.maxpool_relu_bwd(x, dq)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    if kind == "ties":
        assert float((x == 0).mean()) > 0.1 and float((got != 0).mean()) > 0.1      # the case does have zeros and routed gradients


def test_pool_argmax_prefers_the_first_of_equal_maxima():
    x = np.zeros((1, 4, 4, 1), np.float32)
    x[0, 0, 1, 0] = x[0, 1, 0, 0] = x[0, 1, 1, 0] = 3.0
    idx = R.pool_argmax(x)
    assert idx[0, 0, 0, 0] == 1                   # (0, 1) comes first in (row, column) order
    assert idx[0, 1, 1, 0] == 1 * 4 + 1           # window rows 1..3, columns 1..3: (1, 1)
    assert idx[0, 1, 0, 0] == 4                   # rows 1..3, columns -1..1: (1, 0), the padding column never wins


@pytest.mark.parametrize("bands", [3, 4])
def test_stem_layout_round_trip(bands):
    """train_tensors(.., 0) -> .m32 -> master_to_d2(.., freeze_at=0) returns the stem and res2 weights bit for bit; the padding columns
    of the stem's master matrix are zero."""
    spec = EngineSpec(num_classes=2, pixel_mean=(100.0,) * bands, pixel_std=(1.0,) * bands)
    assert spec.in_channels == bands
    W = synthetic_weights(spec, seed=3)
    T = train_tensors(spec, W, 0)
    stem = "backbone.bottom_up.stem.conv1"
    m = T[stem + ".m32"]
    assert m.shape == (64, 256) and m.dtype == np.float32 and (stem + ".s") in T
    pad = R.stem_padding_mask() | (np.arange(256) % STEM_CIN_PAD >= bands)
    assert np.all(m[:, pad] == 0) and np.all(m[:, ~pad] != 0) and int((~pad).sum()) == 49 * bands
    assert STEM_KW_PAD == 8 and STEM_CIN_PAD == 4
    base = {k: np.zeros_like(v) for k, v in W.items()}          # nothing of the result may come from `base`
    for fa in (0, 1):
        Tf = dict(engine_tensors(spec, W, w_dtype=np.float32, fold_bn=False))        # the biases a trainer holds
        Tf.update(train_tensors(spec, W, fa))
        out = master_to_d2(spec, base, lambda name: Tf[name[2:-2] + (".m32" if name.endswith(".w") else ".b")], freeze_at=fa)
        for name, _, _, _, _ in conv_layers(spec):
            if ".res2." in name or (fa == 0 and name == stem):
                assert out[name + ".weight"].shape == W[name + ".weight"].shape
                assert np.array_equal(out[name + ".weight"], W[name + ".weight"].astype(np.float32)), name
        if fa == 1:
            assert not out[stem + ".weight"].any()                 # frozen: left as `base` has it
    assert out[stem + ".weight"].shape == (64, bands, 7, 7)


def test_packed_blob_follows_freeze_at():
    spec = EngineSpec(num_classes=2, precision="fp32")
    W = synthetic_weights(spec, seed=1)
    has = lambda fa, n: (n + ".m32") in packed_tensors(spec, W, train=True, freeze_at=fa)
    assert not has(2, "backbone.bottom_up.res2.0.conv1") and not has(2, "backbone.bottom_up.stem.conv1")
    assert has(1, "backbone.bottom_up.res2.0.conv1") and not has(1, "backbone.bottom_up.stem.conv1")
    assert has(0, "backbone.bottom_up.res2.2.conv3") and has(0, "backbone.bottom_up.stem.conv1")
    assert sorted(packed_tensors(spec, W, train=True)) == sorted(packed_tensors(spec, W, train=True, freeze_at=2))


def test_trainable_layer_counts():
    spec = EngineSpec(num_classes=2)
    n2, n1, n0 = (len(trainable_layers(spec, fa)) for fa in (2, 1, 0))
    res2 = 3 * spec.res_blocks[0] + 1                   # three convolutions per block and res2.0's projection shortcut
    assert n1 == n2 + res2 and n0 == n1 + 1
    assert trainable_layers(spec) == trainable_layers(spec, 2)
    assert trainable_layers(spec, 0)[0] == "backbone.bottom_up.stem.conv1"
    assert [n for n in trainable_layers(spec, 1) if n not in trainable_layers(spec, 2)] == \
        [n for n, _, _, _, _ in conv_layers(spec) if ".res2." in n]


def _yaml(tmp_path, freeze_at):
    p = tmp_path / f"fa_{freeze_at}.yaml"
    p.write_text("MODEL:\n  BACKBONE:\n    FREEZE_AT: %s\n" % freeze_at if freeze_at is not None else "MODEL:\n  MASK_ON: true\n")
    return str(p)


@pytest.mark.parametrize("freeze_at", [0, 1, 2])
def test_solver_accepts_the_implemented_values(tmp_path, freeze_at):
    sv = train_model.load_solver(_yaml(tmp_path, freeze_at))
    assert sv["freeze_at"] == freeze_at
    train_model.validate_solver(sv)


def test_solver_default_is_two(tmp_path):
    sv = train_model.load_solver(_yaml(tmp_path, None))
    assert sv["freeze_at"] == 2
    train_model.validate_solver(sv)


@pytest.mark.parametrize("freeze_at", [3, 5, -1])
def test_solver_rejects_other_values_by_name(tmp_path, freeze_at):
    sv = train_model.load_solver(_yaml(tmp_path, freeze_at))
    with pytest.raises(SystemExit) as e:
        train_model.validate_solver(sv)
    assert "FREEZE_AT" in str(e.value) and str(freeze_at) in str(e.value)


def test_reference_yaml_reads_two():
    from tests.test_train_host_cpu import REF_YAML as path
    if not os.path.exists(path):
        return                                   # the reference project is not here: nothing to read
    sv = train_model.load_solver(path)
    assert sv["freeze_at"] == 2
    train_model.validate_solver(sv)


def test_trainer_classes_take_freeze_at():
    import inspect

    from proj_roadsurf_amd import engine
    for cls in (engine.Trainer, engine.MultiScaleTrainer):
        assert inspect.signature(cls.__init__).parameters["freeze_at"].default == 2
    for bad in (3, -1, 5, True, "0", 1.0):
        with pytest.raises(ValueError, match="FREEZE_AT"):
            engine._check_freeze_at(bad)
    assert [engine._check_freeze_at(v) for v in (0, 1, 2)] == [0, 1, 2]
    assert engine.RsTrainOptions._fields_[0][0] == "struct_size" and engine.RsTrainOptions._fields_[1][0] == "freeze_at"


def test_header_declares_the_abi():
    with open(os.path.join(ROOT, "include", "rs_engine.h")) as f:
        h = f.read()
    assert re.search(r"typedef struct rs_train_options \{\s*int32_t struct_size;[^}]*int32_t freeze_at;[^}]*\} rs_train_options;", h)
    assert re.search(r"int rs_trainer_create2\([^;]*const rs_train_options\* opts, rs_trainer\*\* out\);", h)
    for entry in ("rs_op_maxpool3x3s2_bwd", "rs_op_stem_wgrad", "rs_op_stem_wgrad_f32", "rs_trainer_freeze_at"):
        assert re.search(r"\b%s\(" % entry, h), entry
