"""CPU tests of the AWQ workflow (torchao.prototype.awq, quantization/linear_activation_scale.py):
config validation, prepare / convert / prepare_for_loading structure, the quantized weight of a
converted module against the reference's own (tests/golden/awq_*.npz, experiments/
gen_golden_awq.py), loading a checkpoint the reference saved, and the refusals. No GPU compute:
a CPU forward of a converted module raises."""

import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, bf16, load_golden, unpack_u8_nibbles

from torchao import _lib
from torchao.dtypes import AffineQuantizedTensor, TensorCoreTiledAQTTensorImpl
from torchao.prototype.awq import AWQConfig, AWQObservedLinear, AWQObserver, AWQStep
from torchao.quantization import (
    Float8DynamicActivationFloat8WeightConfig,
    Int4WeightOnlyConfig,
    Int8DynamicActivationInt8WeightConfig,
    WeightTensorWithLinearActivationScaleMetadata,
    quantize_,
    to_weight_tensor_with_linear_activation_scale_metadata,
)

FIXTURES = ["awq_N64_K256_g32.npz", "awq_N96_K1024_g64.npz", "awq_N48_K512_g128.npz"]


def _linear(rec):
    N, K = int(rec["N"]), int(rec["K"])
    lin = torch.nn.Linear(K, N, bias=True, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        lin.bias.copy_(bf16(rec["bias"]))
    return lin


def test_config_validation_and_defaults():
    base = Int4WeightOnlyConfig(group_size=32)
    for step in ("prepare", "CONVERT", "Prepare_For_Loading", AWQStep.PREPARE):
        cfg = AWQConfig(base, step=step)
        assert cfg.step in [s.value for s in AWQStep]
        assert cfg.step == AWQStep(cfg.step)
    cfg = AWQConfig(base, step="convert")
    assert cfg.scale_search_space_size == 20 and cfg.base_config is base
    with pytest.raises(ValueError, match="calibrate"):
        AWQConfig(base, step="calibrate")
    assert [s.value for s in AWQStep] == ["prepare", "convert", "prepare_for_loading"]


def test_prepare_swaps_in_an_observed_linear_that_records():
    rec = load_golden(FIXTURES[0])
    lin = _linear(rec)
    model = torch.nn.Sequential(lin)
    quantize_(model, AWQConfig(Int4WeightOnlyConfig(group_size=32), step="prepare",
                               scale_search_space_size=7))
    obs_lin = model[0]
    assert isinstance(obs_lin, AWQObservedLinear) and isinstance(obs_lin.act_obs, AWQObserver)
    assert obs_lin.weight is lin.weight and obs_lin.bias is lin.bias
    assert obs_lin.act_obs.scale_options == 7 and obs_lin.act_obs.losses == []
    x = bf16(rec["x"])
    y = model(x)
    assert torch.equal(y, F.linear(x, lin.weight, lin.bias))
    model(x[:2])
    assert len(obs_lin.act_obs.inputs) == 2
    assert torch.equal(obs_lin.act_obs.inputs[0], x) and torch.equal(obs_lin.act_obs.inputs[1], x[:2])


def test_convert_skips_a_module_that_was_not_observed():
    lin = torch.nn.Linear(64, 32, dtype=torch.bfloat16)
    w = lin.weight
    model = torch.nn.Sequential(lin)
    quantize_(model, AWQConfig(Int4WeightOnlyConfig(group_size=32), step="convert"))
    assert model[0] is lin and lin.weight is w and type(lin.weight) is torch.nn.Parameter


@pytest.mark.parametrize("name", FIXTURES)
def test_convert_with_the_fixture_scale_matches_the_reference_bit_for_bit(name):
    """With the search replaced by the reference's size-5 scale, convert on the CPU quantizes
    weight * scale to the reference's codes, scales and zeros; the wrapper holds that scale and the
    plain nn.Linear keeps the bias."""
    rec = load_golden(name)
    N, K, g = int(rec["N"]), int(rec["K"]), int(rec["g"])
    scale = bf16(rec["scale_5"])
    lin = _linear(rec)
    bias = lin.bias
    model = torch.nn.Sequential(lin)
    base = Int4WeightOnlyConfig(group_size=g)
    quantize_(model, AWQConfig(base, step="prepare", scale_search_space_size=5))
    model[0].act_obs.calculate_qparams = lambda: scale.clone()
    quantize_(model, AWQConfig(base, step="convert", scale_search_space_size=5))
    out = model[0]
    assert type(out) is torch.nn.Linear and out.bias is bias
    assert (out.in_features, out.out_features) == (K, N)
    w = out.weight
    assert isinstance(w, WeightTensorWithLinearActivationScaleMetadata)
    assert tuple(w.shape) == (N, K) and w.dtype == torch.bfloat16
    assert torch.equal(w.scale, scale)
    inner = w.original_weight_tensor
    assert isinstance(inner, AffineQuantizedTensor)
    assert isinstance(inner.tensor_impl, TensorCoreTiledAQTTensorImpl)
    q, s, z = inner.tensor_impl.get_plain()
    assert torch.equal(q, torch.from_numpy(rec["q"].astype("int32")))
    assert torch.equal(s, bf16(rec["s"])) and torch.equal(z, bf16(rec["z"]))
    assert "WeightTensorWithLinearActivationScaleMetadata" in repr(out) or "weight=" in repr(out)
    # no number comes out of a CPU forward
    with pytest.raises((NotImplementedError, RuntimeError)):
        model(bf16(rec["x"]))


def _ckpt_expected():
    rec = load_golden("awq_refckpt_N48_K352_g32.npz")
    q = unpack_u8_nibbles(rec["q_u8"])
    return rec, q, bf16(rec["s"]), bf16(rec["z"]), bf16(rec["scale"])


def _check_ckpt_weight(w, q, s, z, scale):
    assert isinstance(w, WeightTensorWithLinearActivationScaleMetadata)
    assert torch.equal(w.scale, scale)
    qq, ss, zz = w.original_weight_tensor.tensor_impl.get_plain()
    assert torch.equal(qq, q) and torch.equal(ss, s) and torch.equal(zz, z)


def test_reference_saved_checkpoint_loads_weights_only():
    """A state_dict the reference pickled (its wrapper class around its TensorCoreTiledLayout
    AQT) loads with weights_only=True, directly and into a prepare_for_loading module, by assign
    and by copy_, with bytes equal to the recorded numbers."""
    import torchao.ops as tops

    rec, q, s, z, scale = _ckpt_expected()
    path = os.path.join(ROOT, "tests", "golden", "awq_refckpt_N48_K352_g32.pt")
    with tops.checkpoint_tile_format(str(rec["fmt"])):
        sd = torch.load(path, weights_only=True)
    N, K, g = int(rec["N"]), int(rec["K"]), int(rec["g"])
    assert tuple(sd["weight"].shape) == (N, K)
    _check_ckpt_weight(sd["weight"], q, s, z, scale)

    for assign in (True, False):
        lin = torch.nn.Linear(K, N, bias="bias" in sd, dtype=torch.bfloat16)
        model = torch.nn.Sequential(lin)
        quantize_(model, AWQConfig(Int4WeightOnlyConfig(group_size=g), step="prepare_for_loading"))
        assert type(model[0]) is torch.nn.Linear
        w0 = model[0].weight
        assert isinstance(w0, WeightTensorWithLinearActivationScaleMetadata)
        assert tuple(w0.scale.shape) == (K,) and w0.scale.dtype == torch.bfloat16
        model[0].load_state_dict(sd, assign=assign)
        _check_ckpt_weight(model[0].weight, q, s, z, scale)
        with pytest.raises((NotImplementedError, RuntimeError)):
            model(torch.ones(1, K, dtype=torch.bfloat16))


def test_wrapper_tensor_ops():
    """detach / alias / _apply_fn_to_data / to / t / slice go to the inner tensor; the scale
    travels with it."""
    rec = load_golden(FIXTURES[0])
    N, K, g = int(rec["N"]), int(rec["K"]), int(rec["g"])
    lin = _linear(rec)
    quantize_(lin, Int4WeightOnlyConfig(group_size=g))
    scale = bf16(rec["scale_5"])
    w = to_weight_tensor_with_linear_activation_scale_metadata(lin.weight.detach(), scale)
    d = w.detach()
    assert isinstance(d, type(w)) and torch.equal(d.scale, scale)
    a = torch.ops.aten.alias(w)
    assert isinstance(a, type(w))
    c = w._apply_fn_to_data(torch.clone)
    assert c.scale.data_ptr() != w.scale.data_ptr() and torch.equal(c.scale, scale)
    t = w.to("cpu")
    assert isinstance(t, type(w)) and t.device.type == "cpu"
    assert isinstance(w.t(), type(w))
    r = w[:16]
    assert isinstance(r, type(w)) and tuple(r.shape) == (16, K) and torch.equal(r.scale, scale)
    q, _, _ = w.original_weight_tensor.tensor_impl.get_plain()
    assert torch.equal(r.original_weight_tensor.tensor_impl.get_plain()[0], q[:16])
    names, attrs = w.__tensor_flatten__()
    assert names == ["original_weight_tensor", "scale"] and attrs == []
    # a plain inner weight on the CPU takes x / scale and the float linear
    p = to_weight_tensor_with_linear_activation_scale_metadata(bf16(rec["w"]), scale)
    x = bf16(rec["x"])
    assert torch.equal(F.linear(x, p), F.linear(x / scale, bf16(rec["w"])))


@pytest.mark.parametrize("step", ["prepare", "prepare_for_loading"])
def test_refusals_leave_the_module_untouched(step):
    lin = torch.nn.Linear(64, 32, dtype=torch.bfloat16)
    w = lin.weight
    for base in (Int8DynamicActivationInt8WeightConfig(),
                 Float8DynamicActivationFloat8WeightConfig()):
        model = torch.nn.Sequential(lin)
        with pytest.raises(NotImplementedError, match="Int4WeightOnlyConfig"):
            quantize_(model, AWQConfig(base, step=step))
        assert model[0] is lin and lin.weight is w

    class Experts(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.zeros(2, 32, 64, dtype=torch.bfloat16))
            self.bias = None

    moe = Experts()
    w3 = moe.weight
    model = torch.nn.Sequential(moe)
    with pytest.raises(NotImplementedError, match="3-D"):
        quantize_(model, AWQConfig(Int4WeightOnlyConfig(group_size=32), step=step),
                  filter_fn=lambda m, fqn: isinstance(m, Experts))
    assert model[0] is moe and moe.weight is w3


def test_convert_refuses_an_observed_activation_quantizing_base():
    lin = torch.nn.Linear(64, 32, dtype=torch.bfloat16)
    obs = AWQObserver(lin.weight, lin.bias, Int8DynamicActivationInt8WeightConfig(), 3)
    observed = AWQObservedLinear.from_float(lin, obs)
    model = torch.nn.Sequential(observed)
    with pytest.raises(NotImplementedError, match="weight-only"):
        quantize_(model, AWQConfig(Int8DynamicActivationInt8WeightConfig(), step="convert"))
    assert model[0] is observed and observed.weight is lin.weight


def test_calculate_qparams_on_cpu_raises_from_the_inner_op():
    rec = load_golden(FIXTURES[0])
    lin = _linear(rec)
    obs = AWQObserver(lin.weight, lin.bias, Int4WeightOnlyConfig(group_size=32), 3)
    obs(bf16(rec["calib"]), None)
    with pytest.raises((NotImplementedError, RuntimeError)):
        obs.calculate_qparams()


def test_new_c_abi_entries_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "torchao_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("tao_act_prescale_bf16", "tao_int4wo_prescaled_linear_bf16",
                 "tao_int4wo_prescaled_linear_fused"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.exported_symbols()
    assert _lib.is_available(), _lib.load_error()
    assert _lib.lib().tao_act_prescale_bf16.argtypes is not None


def test_one_launch_routing_query():
    """tao_int4wo_prescaled_linear_fused: one token, no bias, K <= 4096, N * K <= 2^24."""
    fused = _lib.lib().tao_int4wo_prescaled_linear_fused
    assert fused(1, 4096, 4096, 0) == 1 and fused(1, 40, 352, 0) == 1 and fused(1, 8192, 2048, 0) == 1
    assert fused(1, 1024, 8192, 0) == 0 and fused(1, 16, 4128, 0) == 0
    assert fused(1, 4104, 4096, 0) == 0 and fused(1, 6144, 4096, 0) == 0
    assert fused(2, 40, 352, 0) == 0 and fused(0, 40, 352, 0) == 0 and fused(1, 40, 352, 1) == 0


def test_ops_are_defined_with_fake_kernels_and_no_cpu_kernel():
    import torchao.ops  # noqa: F401

    for name in ("act_prescale", "int4_prescaled_linear"):
        table = torch._C._dispatch_dump(f"torchao::{name}")
        lines = table.splitlines()
        assert any(ln.startswith("Meta:") for ln in lines), table
        assert not any(ln.startswith("CPU:") for ln in lines), table
    x = torch.ones(2, 64, dtype=torch.bfloat16)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.torchao.act_prescale(x, torch.ones(64, dtype=torch.bfloat16))
    y = torch.ops.torchao.act_prescale(x.to("meta"), torch.ones(64, dtype=torch.bfloat16, device="meta"))
    assert tuple(y.shape) == (2, 64) and y.dtype == torch.bfloat16
