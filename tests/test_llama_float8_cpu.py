"""float8 in the Llama harness, the parts that need no GPU: the ``-q`` strings of
``apply_quantization`` and the weight criteria of the fused float8 decode dispatch
(``_fp8wo_parts`` / ``_fp8dq_parts`` in torchao/_models/llama/model.py)."""

import pytest
import torch
import torch.nn as nn

from torchao._models.llama import model as M
from torchao._models.llama.generate import apply_quantization
from torchao._models.llama.model import ModelArgs, Transformer
from torchao.dtypes.affine_quantized_tensor import AffineQuantizedTensor
from torchao.dtypes.floatx.float8_layout import Float8Layout
from torchao.quantization import (
    Float8DynamicActivationFloat8WeightConfig,
    Float8WeightOnlyConfig,
    Int8WeightOnlyConfig,
    PerRow,
    quantize_,
)
from torchao.quantization.linear_activation_quantized_tensor import (
    LinearActivationQuantizedTensor,
)


def _tiny(seed=0):
    torch.manual_seed(seed)
    cfg = ModelArgs(dim=64, n_layer=1, n_head=2, vocab_size=96, intermediate_size=128,
                    block_size=32)
    return Transformer(cfg).to(torch.bfloat16).eval()


def _linears(model):
    return [m for m in model.modules() if isinstance(m, nn.Linear)]


def _linear(K=64, N=32, bias=False):
    torch.manual_seed(1)
    return nn.Linear(K, N, bias=bias, dtype=torch.bfloat16)


def test_float8wo_string():
    model = apply_quantization(_tiny(), "float8wo")
    lins = _linears(model)
    assert len(lins) == 6  # wqkv, wo, w1, w2, w3, output
    for lin in lins:
        w = lin.weight
        assert isinstance(w, AffineQuantizedTensor) and isinstance(w._layout, Float8Layout)
        assert w.tensor_impl.float8_data.dtype == torch.float8_e4m3fn
        assert w.tensor_impl.scale.dtype == torch.float32
        assert w.tensor_impl.scale.numel() == lin.out_features


def test_float8dq_row_string():
    model = apply_quantization(_tiny(), "float8dq-row")
    for lin in _linears(model):
        w = lin.weight
        assert isinstance(w, LinearActivationQuantizedTensor)
        assert set(w.quant_kwargs) == {"activation_granularity", "activation_dtype"}
        assert isinstance(w.quant_kwargs["activation_granularity"], PerRow)
        assert w.quant_kwargs["activation_dtype"] == torch.float8_e4m3fn
        inner = w.original_weight_tensor
        assert isinstance(inner, AffineQuantizedTensor) and isinstance(inner._layout, Float8Layout)
        assert inner._layout.mm_config is not None


@pytest.mark.parametrize("q", ["float8dq", "float8dq-tensor"])
def test_per_tensor_strings_raise_the_configs_error(q):
    """The reference parses both as PerTensor(); the config refuses it and names PerRow. It is
    neither turned into a ValueError nor quietly run per row."""
    model = _tiny()
    with pytest.raises(NotImplementedError, match="PerRow"):
        apply_quantization(model, q)
    assert all(type(lin.weight) is nn.Parameter for lin in _linears(model))


@pytest.mark.parametrize("q", ["float9", "float8", "float8wo-row", "float8dq-col", "fp8wo"])
def test_unknown_strings_still_raise_value_error(q):
    with pytest.raises(ValueError, match="unsupported quantization"):
        apply_quantization(_tiny(), q)


def test_existing_strings_behave_as_before():
    model = _tiny()
    assert apply_quantization(model, None) is model and apply_quantization(model, "") is model
    assert all(type(lin.weight) is nn.Parameter for lin in _linears(model))
    apply_quantization(model, "int8wo")
    for lin in _linears(model):
        assert isinstance(lin.weight, AffineQuantizedTensor)
        assert lin.weight.tensor_impl.int_data.dtype == torch.int8
    model = apply_quantization(_tiny(), "int8dq")
    for lin in _linears(model):
        w = lin.weight
        assert isinstance(w, LinearActivationQuantizedTensor) and not w.quant_kwargs
        assert w.original_weight_tensor.tensor_impl.int_data.dtype == torch.int8


def test_fp8_parts_refuse_what_the_kernels_cannot_read():
    plain = _linear()
    assert M._fp8wo_parts(plain) is None and M._fp8dq_parts(plain) is None
    assert M._fp8wo_parts(None) is None and M._fp8dq_parts(None) is None
    i8 = _linear()
    quantize_(i8, Int8WeightOnlyConfig())
    assert M._fp8wo_parts(i8) is None and M._fp8dq_parts(i8) is None
    for cfg, parts, other in (
            (Float8WeightOnlyConfig(), M._fp8wo_parts, M._fp8dq_parts),
            (Float8DynamicActivationFloat8WeightConfig(granularity=PerRow()), M._fp8dq_parts,
             M._fp8wo_parts)):
        lin = _linear()
        quantize_(lin, cfg)
        assert parts(lin) is None  # a CPU weight
        assert other(lin) is None  # the other recipe's weight
        biased = _linear(bias=True)
        quantize_(biased, cfg)
        assert parts(biased) is None
        cast = _linear()
        quantize_(cast, cfg)
        w = cast.weight
        inner = w.original_weight_tensor if isinstance(w, LinearActivationQuantizedTensor) else w
        inner.tensor_impl.scale = inner.tensor_impl.scale.to(torch.bfloat16)
        assert parts(cast) is None
        # the integer dispatches do not take a float8 weight either
        assert M._int4_parts(lin) is None
        assert M._int8wo_parts(lin) is None
        assert M._int8dq_parts(lin) is None


def test_fused_decode_declines_two_tokens_and_cpu_weights():
    lin = _linear()
    quantize_(lin, Float8WeightOnlyConfig())
    assert M._fused_decode(torch.zeros(2, 64, dtype=torch.bfloat16), lin) is None
    assert M._fused_decode(torch.zeros(1, 1, 64, dtype=torch.bfloat16), lin) is None
