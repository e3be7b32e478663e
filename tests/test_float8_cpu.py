"""CPU tests of the float8 (e4m3fn) weight-only workflow: the torch-op primitives against the
reference fixtures byte for byte, quantize_ on a CPU nn.Linear, checkpoint interchange with the
reference, the tensor-subclass mechanics, the config's refusals and the op registration. No GPU
compute is invoked here."""

import io
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, bf16, golden_files, load_golden

import exact_inputs_fp8 as E8
from exact_inputs_fp8 import rel_l2_finite, same_bf16, same_codes

from torchao.dtypes import (
    AffineQuantizedTensor,
    Float8AQTTensorImpl,
    Float8Layout,
    Float8MMConfig,
    to_affine_quantized_floatx,
)
from torchao.quantization import Float8WeightOnlyConfig, float8_weight_only, quantize_
from torchao.quantization.quant_primitives import (
    _choose_scale_float8,
    _dequantize_affine_float8,
    _expand_scale_to_tensor_shape,
    _quantize_affine_float8,
)

FP8 = torch.float8_e4m3fn
FIXTURES = golden_files("float8wo_N")
CKPT = "float8wo_refckpt_v1_N32_K64"


def _u8(t):
    return t.view(torch.uint8)


def test_fixture_files_present():
    assert FIXTURES == ["float8wo_N64_K256.npz", "float8wo_N96_K1024.npz"]
    assert any(int(load_golden(f)["zero_row"]) >= 0 for f in FIXTURES)


@pytest.mark.parametrize("fname", FIXTURES)
def test_primitives_match_reference_byte_for_byte(fname):
    rec = load_golden(fname)
    N, K = int(rec["N"]), int(rec["K"])
    w = bf16(rec["w"])
    s = _choose_scale_float8(w, block_size=(1, K), float8_dtype=FP8)
    assert s.dtype == torch.float32 and tuple(s.shape) == (N, 1)
    assert torch.equal(s.reshape(-1), torch.from_numpy(rec["s"]))
    q = _quantize_affine_float8(w, s, FP8)
    assert q.dtype == FP8
    assert same_codes(_u8(q), torch.from_numpy(rec["q"]))
    dq = _dequantize_affine_float8(q, s, torch.bfloat16)
    assert same_bf16(dq, bf16(rec["w_dequant"]))
    zr = int(rec["zero_row"])
    if zr >= 0:  # no eps: scale exactly 0, NaN codes, NaN dequant
        assert float(s[zr]) == 0.0
        assert bool(((_u8(q)[zr] & 0x7F) == 0x7F).all())
        assert bool(dq[zr].isnan().all())
        assert int(dq.isnan().sum()) == K


@pytest.mark.parametrize("fname", FIXTURES)
def test_reference_output_meets_the_float64_bar(fname):
    """The recorded reference-module output is itself within the project's bar against float64
    (rel-L2 <= 4e-3, the int4-against-fp32 bar), so tests/test_gpu_float8.py may hold the HIP
    linear to the bar of 1e-2 against it."""
    rec = load_golden(fname)
    y64 = torch.from_numpy(rec["y64"]) + bf16(rec["bias"]).double()
    for M in (1, 3, 5):
        assert rel_l2_finite(bf16(rec["y_ref"])[:M], y64[:M]) <= 4e-3


def test_primitives_scope_and_scale_expansion():
    w = torch.randn(4, 64)
    with pytest.raises(NotImplementedError):
        _choose_scale_float8(w, (1, 64), hp_value_lb=1e-3)
    with pytest.raises(NotImplementedError):
        _choose_scale_float8(w, (1, 64), scale_dtype=torch.float8_e8m0fnu)
    s = _choose_scale_float8(w, (), float8_dtype=FP8)
    assert s.dim() == 0 and float(s) == float(w.abs().max() / 448.0)
    s2 = _choose_scale_float8(w, (1, 32))
    assert tuple(s2.shape) == (4, 2)
    ex = _expand_scale_to_tensor_shape(s2, w.shape)
    assert tuple(ex.shape) == (4, 64) and torch.equal(ex[:, :32], s2[:, :1].expand(4, 32))
    with pytest.raises(ValueError):
        _expand_scale_to_tensor_shape(torch.ones(4), w.shape)
    with pytest.raises(ValueError):
        _expand_scale_to_tensor_shape(torch.ones(3, 1), w.shape)
    # fp32 weights: the scale division stays in fp32
    assert torch.equal(_choose_scale_float8(w, (1, 64)), w.abs().amax(1, keepdim=True) / 448.0)


def _quantized_linear(rec, bias=True):
    N, K = int(rec["N"]), int(rec["K"])
    lin = torch.nn.Linear(K, N, bias=bias, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        if bias:
            lin.bias.copy_(bf16(rec["bias"]))
    quantize_(lin, Float8WeightOnlyConfig())
    return lin


@pytest.mark.parametrize("fname", FIXTURES)
def test_quantize_cpu_linear_reproduces_reference(fname):
    rec = load_golden(fname)
    N, K = int(rec["N"]), int(rec["K"])
    lin = _quantized_linear(rec)
    w = lin.weight
    assert isinstance(w, AffineQuantizedTensor)
    assert isinstance(w._layout, Float8Layout) and w._layout.mm_config is None
    assert isinstance(w.tensor_impl, Float8AQTTensorImpl)
    assert w.shape == (N, K) and w.dtype == torch.bfloat16 and w.block_size == (1, K)
    assert w.quant_min is None and w.quant_max is None
    data, scale, zp = w.tensor_impl.get_plain()
    assert zp is None and data.dtype == FP8 and scale.dtype == torch.float32
    assert tuple(scale.shape) == (N, 1) and not w.tensor_impl.transposed
    assert same_codes(_u8(data), torch.from_numpy(rec["q"]))
    assert torch.equal(scale.reshape(-1), torch.from_numpy(rec["s"]))
    assert same_bf16(w.dequantize(), bf16(rec["w_dequant"]))


def test_extra_repr_matches_reference_format():
    lin = _quantized_linear(load_golden(FIXTURES[0]))
    assert repr(lin) == (
        "Linear(in_features=256, out_features=64, weight=AffineQuantizedTensor("
        "shape=torch.Size([64, 256]), block_size=(1, 256), device=cpu, "
        "_layout=Float8Layout(mm_config=None), tensor_impl_dtype=torch.float8_e4m3fn, "
        "quant_min=None, quant_max=None))"
    )


def test_reference_checkpoint_loads_weights_only():
    """A state_dict pickled by the REFERENCE's own classes (tools/gen_golden_float8.py) loads
    with weights_only=True into this package: same class paths, attribute names and flatten
    order."""
    rec = load_golden(CKPT + ".npz")
    N, K = int(rec["N"]), int(rec["K"])
    sd = torch.load(os.path.join(GOLDEN, CKPT + ".pt"), weights_only=True)
    aqt = sd["weight"]
    assert isinstance(aqt, AffineQuantizedTensor)
    assert isinstance(aqt.tensor_impl, Float8AQTTensorImpl)
    assert isinstance(aqt._layout, Float8Layout)
    assert tuple(aqt.shape) == (N, K) and aqt.block_size == (1, K)
    assert aqt.tensor_impl.__tensor_flatten__()[0] == ["float8_data", "scale"]
    assert torch.equal(_u8(aqt.tensor_impl.float8_data), torch.from_numpy(rec["q"]))
    assert torch.equal(aqt.tensor_impl.scale.reshape(-1), torch.from_numpy(rec["s"]))
    assert aqt.tensor_impl.transposed is False
    assert torch.equal(aqt.dequantize(), bf16(rec["w_dequant"]))
    assert torch.equal(sd["bias"], bf16(rec["bias"]))
    for assign in (False, True):  # into a quantized nn.Linear of this package, both load modes
        lin = torch.nn.Linear(K, N, dtype=torch.bfloat16)
        quantize_(lin, Float8WeightOnlyConfig())
        lin.load_state_dict(sd, assign=assign)
        assert torch.equal(_u8(lin.weight.tensor_impl.float8_data), torch.from_numpy(rec["q"]))
        assert torch.equal(lin.bias, bf16(rec["bias"]))


def test_own_state_dict_roundtrip_weights_only():
    lin = _quantized_linear(load_golden(FIXTURES[1]))
    buf = io.BytesIO()
    torch.save(lin.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, weights_only=True)
    lin2 = torch.nn.Linear(1024, 96, dtype=torch.bfloat16)
    quantize_(lin2, Float8WeightOnlyConfig())
    lin2.load_state_dict(sd, assign=True)
    assert torch.equal(_u8(lin2.weight.tensor_impl.float8_data),
                       _u8(lin.weight.tensor_impl.float8_data))
    assert torch.equal(lin2.weight.tensor_impl.scale, lin.weight.tensor_impl.scale)
    assert torch.equal(lin2.weight.dequantize(), lin.weight.dequantize())


def test_slice_t_clone_detach():
    w = _quantized_linear(load_golden(FIXTURES[1])).weight
    full = w.dequantize()
    rows = w[8:24]
    assert rows.shape == (16, 1024) and tuple(rows.tensor_impl.scale.shape) == (16, 1)
    assert torch.equal(rows.dequantize(), full[8:24])
    cols = torch.ops.aten.slice.Tensor(w, 1, 64, 192, 1)
    assert cols.shape == (96, 128) and cols.block_size == (1, 128)
    assert tuple(cols.tensor_impl.scale.shape) == (96, 1)
    assert torch.equal(cols.dequantize(), full[:, 64:192])
    wt = w.t()
    assert wt.shape == (1024, 96) and wt.tensor_impl.transposed and wt.block_size == (1024, 1)
    assert not w.tensor_impl.transposed  # t() leaves its argument as it was
    assert torch.equal(wt.dequantize(), full.t())
    back = wt.t()
    assert back.shape == (96, 1024) and not back.tensor_impl.transposed
    c = w.detach().clone()
    assert torch.equal(_u8(c.tensor_impl.float8_data), _u8(w.tensor_impl.float8_data))
    assert c.tensor_impl.float8_data.data_ptr() != w.tensor_impl.float8_data.data_ptr()
    assert c.tensor_impl.scale.data_ptr() != w.tensor_impl.scale.data_ptr()
    d = w.detach()
    assert d.tensor_impl.float8_data.data_ptr() == w.tensor_impl.float8_data.data_ptr()
    with torch.no_grad():
        c.tensor_impl.float8_data.view(torch.uint8).zero_()
        c.copy_(w)
    assert torch.equal(c.dequantize(), full)


def test_config_defaults_alias_and_refusals():
    cfg = Float8WeightOnlyConfig()
    assert cfg.version == 1 and cfg.weight_dtype == FP8 and cfg.set_inductor_config is True
    assert float8_weight_only is Float8WeightOnlyConfig
    assert Float8MMConfig() == (False, False, False)
    for bad in (Float8WeightOnlyConfig(version=2),
                Float8WeightOnlyConfig(weight_dtype=torch.float8_e5m2)):
        lin = torch.nn.Linear(64, 8, dtype=torch.bfloat16)
        with pytest.raises(NotImplementedError):
            quantize_(lin, bad)
        assert not isinstance(lin.weight, AffineQuantizedTensor)
    with pytest.raises(NotImplementedError):
        to_affine_quantized_floatx(torch.randn(8, 64), (1, 64), torch.float8_e5m2,
                                   Float8Layout(mm_config=None))


def test_cpu_linear_fails_loudly_no_silent_fallback():
    """The fp8 op has no CPU kernel: a CPU call must raise, never dequantize -> F.linear."""
    lin = _quantized_linear(load_golden(FIXTURES[0]))
    with pytest.raises((NotImplementedError, RuntimeError)):
        lin(torch.randn(1, 256, dtype=torch.bfloat16))
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.torchao.fp8_quantize_rows(torch.randn(4, 64, dtype=torch.bfloat16))
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.torchao.fp8_dequantize(torch.zeros(4, 64).to(FP8), torch.ones(4))


def test_dispatch_pair_is_registered_and_a_plugin_ahead_of_it_wins():
    from torchao.dtypes import (
        deregister_aqt_quantized_linear_dispatch,
        register_aqt_quantized_linear_dispatch,
    )
    from torchao.dtypes import affine_quantized_tensor_ops as ops_mod
    from torchao.dtypes.floatx.float8_layout import (
        _linear_fp_act_fp8_weight_check,
        _linear_fp_act_fp8_weight_impl,
    )

    table = ops_mod._AQT_QLINEAR_DISPATCH_TABLE
    assert table[_linear_fp_act_fp8_weight_check] is _linear_fp_act_fp8_weight_impl
    lin = _quantized_linear(load_golden(FIXTURES[0]), bias=False)
    w = lin.weight
    x = torch.randn(2, 256, dtype=torch.bfloat16)
    assert _linear_fp_act_fp8_weight_check(x, w, None)
    assert _linear_fp_act_fp8_weight_check(x.float(), w, None)
    assert not _linear_fp_act_fp8_weight_check(x.to(torch.int32), w, None)
    assert not _linear_fp_act_fp8_weight_check(x, w.t(), None)
    assert not _linear_fp_act_fp8_weight_check(x, torch.ops.aten.slice.Tensor(w, 1, 0, 128, 1).t(),
                                               None)
    calls = []

    def check(xx, ww, b):
        return isinstance(ww, AffineQuantizedTensor) and isinstance(ww._layout, Float8Layout)

    def impl(xx, ww, b):
        calls.append(1)
        return torch.zeros(*xx.shape[:-1], ww.shape[0], dtype=xx.dtype)

    register_aqt_quantized_linear_dispatch(check, impl)
    items = list(table.items())
    table.clear()
    table[check] = impl
    table.update({k: v for k, v in items if k is not check})
    try:
        y = lin(x)
        assert calls == [1] and torch.count_nonzero(y) == 0
    finally:
        deregister_aqt_quantized_linear_dispatch(check)
    assert check not in table and _linear_fp_act_fp8_weight_check in table


def test_fake_impls_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        x = torch.empty(3, 5, 4096, dtype=torch.bfloat16, device="cuda")
        w8 = torch.empty(512, 4096, dtype=FP8, device="cuda")
        ws = torch.empty(512, dtype=torch.float32, device="cuda")
        y = torch.ops.torchao.fp8_weight_only_linear(x, w8, ws, None)
        assert y.shape == (3, 5, 512) and y.dtype == torch.bfloat16
        wb = torch.empty(512, 4096, dtype=torch.bfloat16, device="cuda")
        q, s = torch.ops.torchao.fp8_quantize_rows(wb)
        assert q.shape == (512, 4096) and q.dtype == FP8
        assert s.shape == (512, 1) and s.dtype == torch.float32
        d = torch.ops.torchao.fp8_dequantize(w8, ws)
        assert d.shape == (512, 4096) and d.dtype == torch.bfloat16
        with pytest.raises(RuntimeError):
            torch.ops.torchao.fp8_weight_only_linear(x, w8.to(torch.int8), ws, None)


def test_fp8_ops_dispatch_to_cpp_kernels():
    from torchao import ops

    served = ops.native_dispatch_float8()
    assert served == {"fp8_weight_only_linear", "fp8_quantize_rows", "fp8_dequantize"}, \
        ops._native_error
    for name in served:
        table = torch._C._dispatch_dump(f"torchao::{name}")
        cuda = [ln for ln in table.splitlines() if ln.startswith("CUDA:")]
        assert cuda and "torch_ops.cpp" in cuda[0], table
        assert any(ln.startswith("Meta:") for ln in table.splitlines()), table


def test_c_abi_argument_checks():
    from torchao import _lib

    lib = _lib.lib()
    rc = lib.tao_fp8wo_linear_bf16(None, None, None, None, None, 1, 8, 48, None)
    assert rc == 1 and b"must be a multiple of 32" in lib.tao_last_error()
    assert lib.tao_fp8wo_linear_bf16(None, None, None, None, None, 0, 8, 64, None) == 0
    rc = lib.tao_fp8_quantize_rows_bf16(None, None, None, 4, 12, None)
    assert rc == 1 and b"multiple of 8" in lib.tao_last_error()
    with pytest.raises(RuntimeError, match="waves_k"):
        _lib.call("tao_tune_fp8_gemv", 4, 8, 2)
    _lib.call("tao_tune_fp8_gemv", 4, 2, 4)
    _lib.call("tao_tune_reset")


@pytest.mark.parametrize("family", E8.FAMILIES)
@pytest.mark.parametrize("M,N,K", [(1, 37, 32), (3, 330, 1056), (8, 37, 8224), (2, 1, 16416),
                                   (70, 72, 3200)])
def test_exact_input_makers_hold_their_conditions(M, N, K, family):
    """The makers assert exactness themselves; here also that the reference is what the header
    formula gives when evaluated in float64 and rounded once."""
    codes, scale, bias, x = E8.make_fp8wo_exact(M, N, K, seed=3, family=family)
    assert codes.dtype == torch.uint8 and scale.dtype == torch.float32
    y = E8.ref_fp8wo(x, codes, scale)
    acc = x.double() @ codes.view(FP8).double().t()
    want = (acc.float() * scale.view(1, -1)).to(torch.bfloat16)
    assert torch.equal(y, want)
    if family == "probe":  # the scaled sum is itself a bf16 number: no rounding hides a code
        assert torch.equal(y.double(), acc * scale.double().view(1, -1))
    yb = E8.ref_fp8wo(x, codes, scale, bias)
    assert torch.equal(yb, (y.float() + bias.float()).to(torch.bfloat16))


def test_every_gpu_shape_has_exact_inputs():
    for M, N, K in E8.fp8_gpu_shapes():
        for family in E8.FAMILIES:
            E8.make_fp8wo_exact(M, N, K, seed=(M * 31 + N * 7 + K) % 1000, family=family)
