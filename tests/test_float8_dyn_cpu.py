"""CPU tests of the float8 dynamic-activation x float8-weight workflow
(Float8DynamicActivationFloat8WeightConfig, granularity PerRow, version 1): the config and its
refusals, the quantized structure and the activation quantisation against the reference fixtures
byte for byte, checkpoint interchange with the reference, the dispatch table, the op registration
and the exact-input makers' own conditions. No GPU compute is invoked here."""

import dataclasses
import io
import os

import pytest
import torch

from conftest import GOLDEN, bf16, golden_files, load_golden

import exact_inputs_fp8dyn as ED
from exact_inputs_fp8 import rel_l2_finite, same_codes

from torchao.dtypes import AffineQuantizedTensor, Float8AQTTensorImpl, Float8Layout, Float8MMConfig
from torchao.quantization import (
    Float8DynamicActivationFloat8WeightConfig,
    Float8WeightOnlyConfig,
    LinearActivationQuantizedTensor,
    PerRow,
    PerTensor,
    float8_dynamic_activation_float8_weight,
    quantize_,
)
from torchao.quantization.quant_api import _input_activation_quant_func_fp8

FP8 = torch.float8_e4m3fn
FIXTURES = golden_files("float8dq_N")
CKPT = "float8dq_refckpt_v1_N32_K64"
CONFIG = Float8DynamicActivationFloat8WeightConfig


def _u8(t):
    return t.view(torch.uint8)


def _linear(rec, bias=True):
    N, K = int(rec["N"]), int(rec["K"])
    lin = torch.nn.Linear(K, N, bias=bias, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        if bias:
            lin.bias.copy_(bf16(rec["bias"]))
    return lin


def test_fixture_files_present():
    assert FIXTURES == ["float8dq_N64_K256.npz", "float8dq_N96_K1024.npz"]
    rec = load_golden(FIXTURES[0])
    assert int(rec["zero_row"]) >= 0 and int(rec["zero_token"]) >= 0


def test_config_defaults_alias_and_granularity():
    assert float8_dynamic_activation_float8_weight is CONFIG
    assert [f.name for f in dataclasses.fields(CONFIG)] == [
        "activation_dtype", "weight_dtype", "granularity", "mm_config", "activation_value_lb",
        "activation_value_ub", "set_inductor_config", "version"]
    c = CONFIG()
    assert c.activation_dtype is FP8 and c.weight_dtype is FP8
    assert c.mm_config == Float8MMConfig(use_fast_accum=True)
    assert c.activation_value_lb is None and c.activation_value_ub is None
    assert c.set_inductor_config is True and c.version == 1
    # granularity is normalised to [activation, weight]; None means per-tensor, as in the reference
    assert c.granularity == [PerTensor(), PerTensor()]
    assert CONFIG(granularity=PerRow()).granularity == [PerRow(), PerRow()]
    assert CONFIG(granularity=(PerRow(), PerRow())).granularity == [PerRow(), PerRow()]
    assert CONFIG(granularity=[PerTensor(), PerTensor()]).granularity == [PerTensor(), PerTensor()]
    with pytest.raises(ValueError):
        CONFIG(granularity=(PerRow(), PerTensor()))
    with pytest.raises(ValueError):
        CONFIG(granularity=(PerRow(),))
    with pytest.raises(ValueError):
        CONFIG(granularity="row")
    assert PerRow.__module__ == "torchao.quantization.granularity"
    assert PerRow() == PerRow() and PerRow() != PerTensor()


@pytest.mark.parametrize("kwargs,dtype", [
    (dict(granularity=PerTensor()), torch.bfloat16),
    (dict(), torch.bfloat16),  # granularity=None: the reference's per-tensor default
    (dict(granularity=PerRow(), version=2), torch.bfloat16),
    (dict(granularity=PerRow(), weight_dtype=torch.float8_e5m2), torch.bfloat16),
    (dict(granularity=PerRow(), activation_dtype=torch.float8_e5m2), torch.bfloat16),
    (dict(granularity=PerRow(), activation_value_lb=1e-3), torch.bfloat16),
    (dict(granularity=PerRow(), activation_value_ub=10.0), torch.bfloat16),
    (dict(granularity=PerRow()), torch.float32),  # PerRow needs a bf16 weight
])
def test_refusals_leave_the_module_untouched(kwargs, dtype):
    lin = torch.nn.Linear(64, 32, dtype=dtype)
    w0 = lin.weight
    before = w0.detach().clone()
    exc = NotImplementedError if dtype is torch.bfloat16 else AssertionError
    with pytest.raises(exc) as ei:
        quantize_(lin, CONFIG(**kwargs))
    if exc is NotImplementedError:  # the message names what is supported
        assert "PerRow" in str(ei.value) and "version=1" in str(ei.value)
    assert lin.weight is w0 and type(lin.weight) is torch.nn.Parameter
    assert torch.equal(lin.weight.detach(), before)
    assert "extra_repr" not in lin.__dict__


def test_fp8_mm_compat_skip():
    """A weight whose N or K is not a multiple of 16 keeps its plain weight (reference
    _fp8_mm_compat)."""
    for K, N in ((40, 16), (64, 24)):
        lin = torch.nn.Linear(K, N, dtype=torch.bfloat16)
        w0 = lin.weight
        quantize_(lin, CONFIG(granularity=PerRow()))
        assert lin.weight is w0 and type(lin.weight) is torch.nn.Parameter
        assert lin(torch.randn(2, K, dtype=torch.bfloat16)).shape == (2, N)


@pytest.mark.parametrize("fname", FIXTURES)
def test_quantized_structure_matches_the_reference(fname):
    rec = load_golden(fname)
    N, K = int(rec["N"]), int(rec["K"])
    lin = _linear(rec)
    quantize_(lin, CONFIG(granularity=PerRow()))
    w = lin.weight
    assert isinstance(w, LinearActivationQuantizedTensor)
    assert w.input_quant_func is _input_activation_quant_func_fp8
    assert w.quant_kwargs == {"activation_granularity": PerRow(), "activation_dtype": FP8}
    inner = w.original_weight_tensor
    assert isinstance(inner, AffineQuantizedTensor)
    assert isinstance(inner.tensor_impl, Float8AQTTensorImpl)
    assert inner._layout == Float8Layout(mm_config=Float8MMConfig(use_fast_accum=True))
    assert inner.block_size == (1, K) and inner.shape == (N, K) and inner.dtype == torch.bfloat16
    impl = inner.tensor_impl
    assert impl.scale.dtype == torch.float32 and not impl.transposed
    assert same_codes(_u8(impl.float8_data), torch.from_numpy(rec["wq"]))
    assert torch.equal(impl.scale.reshape(-1), torch.from_numpy(rec["ws"]))


@pytest.mark.parametrize("fname", FIXTURES)
def test_activation_quant_matches_the_reference(fname):
    rec = load_golden(fname)
    x = bf16(rec["x"])
    for xx in (x, x.view(1, 5, -1)):
        aqt = _input_activation_quant_func_fp8(xx, PerRow(), FP8)
        assert isinstance(aqt, AffineQuantizedTensor) and aqt.shape == xx.shape
        assert aqt._layout == Float8Layout(mm_config=None)
        assert aqt.block_size == (1,) * (xx.dim() - 1) + (xx.shape[-1],)
        impl = aqt.tensor_impl
        assert impl.scale.dtype == torch.float32
        assert same_codes(_u8(impl.float8_data).reshape(5, -1), torch.from_numpy(rec["xq"]))
        assert torch.equal(impl.scale.reshape(-1), torch.from_numpy(rec["xs"]))
    zt = int(rec["zero_token"])
    if zt >= 0:  # no eps: scale exactly 0 and NaN codes
        assert float(rec["xs"][zt]) == 0.0
        assert bool(((torch.from_numpy(rec["xq"])[zt] & 0x7F) == 0x7F).all())
    with pytest.raises(NotImplementedError, match="PerRow"):
        _input_activation_quant_func_fp8(x, PerTensor(), FP8)
    with pytest.raises(AssertionError):
        _input_activation_quant_func_fp8(x.float(), PerRow(), FP8)


@pytest.mark.parametrize("fname", FIXTURES)
def test_float32_formula_meets_the_bar_on_the_fixtures(fname):
    """The header formula evaluated in float32 (products, sum and epilogue) is within the project's
    bar of 4e-3 against its float64 evaluation on the same codes, and so is its bf16 rounding:
    the reference leaves the bar room, tests/test_gpu_float8_dyn.py may hold the kernels to it."""
    rec = load_golden(fname)
    xq = torch.from_numpy(rec["xq"]).view(FP8).float()
    wq = torch.from_numpy(rec["wq"]).view(FP8).float()
    xs, ws = torch.from_numpy(rec["xs"]), torch.from_numpy(rec["ws"])
    y32 = ((xq @ wq.t()) * xs.view(-1, 1)) * ws.view(1, -1) + bf16(rec["bias"]).float()
    y64 = torch.from_numpy(rec["y64"])
    e32, e16 = rel_l2_finite(y32, y64), rel_l2_finite(y32.to(torch.bfloat16), y64)
    print(f"{fname}: float32 formula vs float64 {e32:.3e}, rounded to bf16 {e16:.3e}")
    assert e32 <= 4e-3 and e16 <= 4e-3


def test_reference_checkpoint_loads():
    rec = load_golden(CKPT + ".npz")
    N, K = int(rec["N"]), int(rec["K"])
    sd = torch.load(os.path.join(GOLDEN, CKPT + ".pt"), weights_only=True)
    w = sd["weight"]
    assert isinstance(w, LinearActivationQuantizedTensor)
    assert w.input_quant_func is _input_activation_quant_func_fp8
    assert w.quant_kwargs == {"activation_granularity": PerRow(), "activation_dtype": FP8}
    inner = w.original_weight_tensor
    assert isinstance(inner, AffineQuantizedTensor) and inner.block_size == (1, K)
    assert inner._layout == Float8Layout(mm_config=Float8MMConfig(use_fast_accum=True))
    assert same_codes(_u8(inner.tensor_impl.float8_data), torch.from_numpy(rec["wq"]))
    assert torch.equal(inner.tensor_impl.scale.reshape(-1), torch.from_numpy(rec["ws"]))
    # assign
    lin = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    lin.load_state_dict(sd, assign=True)
    assert isinstance(lin.weight, LinearActivationQuantizedTensor)
    assert torch.equal(lin.bias, bf16(rec["bias"]))
    # copy into a module quantized here
    lin2 = torch.nn.Linear(K, N, dtype=torch.bfloat16)
    quantize_(lin2, CONFIG(granularity=PerRow()))
    lin2.load_state_dict(sd)
    got = lin2.weight.original_weight_tensor.tensor_impl
    assert same_codes(_u8(got.float8_data), torch.from_numpy(rec["wq"]))
    assert torch.equal(got.scale.reshape(-1), torch.from_numpy(rec["ws"]))
    # the reference's repr of the quantized module (the function's address aside)
    import re

    strip = lambda s: re.sub(r" at 0x[0-9a-f]+", "", s)  # noqa: E731
    quantize_(lin := torch.nn.Linear(K, N, dtype=torch.bfloat16), CONFIG(granularity=PerRow()))
    assert strip(repr(lin)) == strip(str(rec["repr"]))


def test_own_state_dict_round_trip():
    rec = load_golden(FIXTURES[0])
    lin = _linear(rec)
    quantize_(lin, CONFIG(granularity=PerRow()))
    buf = io.BytesIO()
    torch.save(lin.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=True)
    lin2 = torch.nn.Linear(int(rec["K"]), int(rec["N"]), dtype=torch.bfloat16)
    lin2.load_state_dict(sd, assign=True)
    a = lin.weight.original_weight_tensor.tensor_impl
    b = lin2.weight.original_weight_tensor.tensor_impl
    assert same_codes(_u8(b.float8_data), _u8(a.float8_data)) and torch.equal(a.scale, b.scale)
    assert lin2.weight.quant_kwargs == lin.weight.quant_kwargs


def test_dispatch_pair_registered_and_weight_only_pair_still_wins():
    from torchao.dtypes import affine_quantized_tensor_ops as ops_mod
    from torchao.dtypes.floatx.float8_layout import (
        _linear_fp8_act_fp8_weight_check,
        _linear_fp8_act_fp8_weight_impl,
        _linear_fp_act_fp8_weight_check,
    )

    table = ops_mod._AQT_QLINEAR_DISPATCH_TABLE
    assert table[_linear_fp8_act_fp8_weight_check] is _linear_fp8_act_fp8_weight_impl
    rec = load_golden(FIXTURES[0])
    K = int(rec["K"])
    dyn = _linear(rec)
    quantize_(dyn, CONFIG(granularity=PerRow()))
    wo = _linear(rec)
    quantize_(wo, Float8WeightOnlyConfig())
    x = bf16(rec["x"])
    qx = _input_activation_quant_func_fp8(x, PerRow(), FP8)
    w_dyn = dyn.weight.original_weight_tensor
    assert _linear_fp8_act_fp8_weight_check(qx, w_dyn, None)
    assert not _linear_fp8_act_fp8_weight_check(x, w_dyn, None)
    assert not _linear_fp_act_fp8_weight_check(qx, w_dyn, None)
    # a plain bf16 input to a weight-only tensor: the weight-only pair, not the new one
    first = next(c for c in table if c(x, wo.weight, None))
    assert first is _linear_fp_act_fp8_weight_check
    assert not _linear_fp8_act_fp8_weight_check(x, wo.weight, None)
    # the impl refuses a transposed weight and per-tensor blocks
    with pytest.raises(NotImplementedError, match="transposed"):
        _linear_fp8_act_fp8_weight_impl(qx, w_dyn.t(), None)
    from torchao.dtypes import to_affine_quantized_floatx

    pt = to_affine_quantized_floatx(x, x.shape, FP8, Float8Layout(mm_config=None),
                                    scale_dtype=torch.float32)
    assert _linear_fp8_act_fp8_weight_check(pt, w_dyn, None)
    with pytest.raises(NotImplementedError, match="per-row"):
        _linear_fp8_act_fp8_weight_impl(pt, w_dyn, None)
    assert K == x.shape[1]


def test_cpu_call_raises():
    rec = load_golden(FIXTURES[0])
    lin = _linear(rec)
    quantize_(lin, CONFIG(granularity=PerRow()))
    with pytest.raises((NotImplementedError, RuntimeError)):
        lin(bf16(rec["x"]))
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.torchao.fp8_dyn_linear(bf16(rec["x"]), torch.from_numpy(rec["wq"]).view(FP8),
                                         torch.from_numpy(rec["ws"]), None)


def test_op_sets_and_bindings():
    from torchao import _lib, ops

    assert ops.native_dispatch_float8_dyn() == {"fp8_scaled_mm", "fp8_dyn_linear"}
    assert ops.native_dispatch_float8() == {"fp8_weight_only_linear", "fp8_quantize_rows",
                                            "fp8_dequantize"}
    assert ops.native_dispatch() == {"int4_weight_only_linear", "int8_weight_only_linear",
                                     "int8_quantize_per_token", "int8_scaled_mm", "int8_dyn_linear"}
    for name in ("fp8_scaled_mm", "fp8_dyn_linear"):
        assert hasattr(torch.ops.torchao, name)
    # argument validation happens before any device work
    lib = _lib.lib()
    assert lib.tao_fp8_scaled_mm_bf16(None, None, None, None, None, None, 2, 16, 40, None) == 1
    assert b"multiple of 16" in lib.tao_last_error()
    assert lib.tao_fp8_dyn_linear_bf16(None, None, None, None, None, 2, 16, 64, None) == 1
    assert b"one token" in lib.tao_last_error()
    assert lib.tao_fp8_scaled_mm_bf16(None, None, None, None, None, None, 0, 16, 64, None) == 0
    with pytest.raises(RuntimeError, match="fp8dyn mfma"):
        _lib.call("tao_tune_fp8dyn_mfma", 2)
    _lib.call("tao_tune_fp8dyn_mfma", 1)
    _lib.call("tao_tune_reset")
    # fake impls
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        xq = torch.empty(2, 3, 64, dtype=FP8)
        w = torch.empty(32, 64, dtype=FP8)
        y = torch.ops.torchao.fp8_scaled_mm(xq, torch.empty(6), w, torch.empty(32), None)
        assert y.shape == (2, 3, 32) and y.dtype == torch.bfloat16
        y = torch.ops.torchao.fp8_dyn_linear(torch.empty(5, 64, dtype=torch.bfloat16), w,
                                             torch.empty(32), None)
        assert y.shape == (5, 32) and y.dtype == torch.bfloat16


@pytest.mark.parametrize("family", ED.FAMILIES)
@pytest.mark.parametrize("M,N,K", [(1, 37, 16), (5, 37, 112), (33, 80, 1040), (8, 1, 4112),
                                   (128, 16, 384)])
def test_exact_input_makers_hold_their_conditions(M, N, K, family):
    xq, xs, wq, ws, bias = ED.make_fp8dyn_exact(M, N, K, 3, family)
    assert xq.dtype == torch.uint8 and xq.shape == (M, K) and wq.shape == (N, K)
    assert xs.dtype == torch.float32 and ws.dtype == torch.float32 and bool((xs > 0).all())
    assert not bool(ED.decode(xq).isnan().any()) and not bool(ED.decode(wq).isnan().any())
    want = ED.ref_fp8dyn(xq, xs, wq, ws, bias)
    assert want.dtype == torch.bfloat16 and want.shape == (M, N)
    # the float64 evaluation of the formula rounds to the same bf16 wherever fp32 was exact
    if family == "probe":  # power-of-two scales: every step of the epilogue is exact
        y64 = ED.exact_acc(xq, wq) * xs.double().view(-1, 1) * ws.double().view(1, -1)
        assert torch.equal(ED.ref_fp8dyn(xq, xs, wq, ws), y64.to(torch.bfloat16))


def test_identity_token_maker():
    from torchao.quantization.quant_primitives import _choose_scale_float8, _quantize_affine_float8

    for K in (16, 1040):
        xb, codes, scale, wq, ws, bias = ED.make_identity_token(37, K, 4)
        s = _choose_scale_float8(xb, block_size=(1, K), float8_dtype=FP8)
        q = _quantize_affine_float8(xb, s, FP8)
        assert torch.equal(s.reshape(-1), scale) and torch.equal(_u8(q), codes)
