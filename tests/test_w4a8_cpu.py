"""CPU tests of the W4A8 workflow (Int8DynamicActivationInt4WeightConfig with
CutlassInt4PackedLayout: per-token int8 activations x per-channel int4 weights packed two per byte):
the config and its refusals, the quantized structure, codes, packed bytes and scales against the
reference fixtures byte for byte (experiments/gen_golden_w4a8.py), checkpoint interchange with the
reference, the op registration and the plain-torch CPU forward. No GPU compute is invoked here."""

import dataclasses
import os

import pytest
import torch

from conftest import GOLDEN, bf16, golden_files, load_golden

from torchao import _lib, ops
from torchao.dtypes import (
    AffineQuantizedTensor,
    CutlassInt4PackedLayout,
    Int4PackedTensorImpl,
    PlainLayout,
    TensorCoreTiledLayout,
)
from torchao.quantization import (
    Int8DynamicActivationInt4WeightConfig,
    LinearActivationQuantizedTensor,
    MappingType,
    ZeroPointDomain,
    int8_dynamic_activation_int4_weight,
    quantize_,
)
from torchao.quantization.quant_api import _int4_symm_cutlass_quant, _int8_symm_cutlass_quant

FIXTURES = ["w4a8_N40_K288.npz", "w4a8_N64_K256.npz", "w4a8_N96_K1024.npz"]
CKPT = "w4a8_refckpt_N32_K64"
CONFIG = Int8DynamicActivationInt4WeightConfig
SYMM = MappingType.SYMMETRIC


def served(**kw):
    return CONFIG(layout=CutlassInt4PackedLayout(), act_mapping_type=SYMM, **kw)


def _linear(rec, dtype=torch.bfloat16):
    N, K = int(rec["N"]), int(rec["K"])
    has_bias = "bias" in rec.files
    lin = torch.nn.Linear(K, N, bias=has_bias, dtype=dtype)
    with torch.no_grad():
        lin.weight.copy_(bf16(rec["w"]))
        if has_bias:
            lin.bias.copy_(bf16(rec["bias"]))
    return lin


def test_fixture_files_present_and_conditions():
    assert golden_files("w4a8_N") == FIXTURES
    for f in os.listdir(GOLDEN):
        if f.startswith("w4a8"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) < (1 << 20), f
    for fname in FIXTURES:
        rec = load_golden(fname)
        x, w = bf16(rec["x"]).float(), bf16(rec["w"]).float()
        xq = torch.from_numpy(rec["xq"])
        p = torch.from_numpy(rec["wq_packed"])
        assert not x[1].any() and not xq[1].any() and not w[1].any() and not p[1].any()
        assert float(x[2].min()) == -float(x[2].abs().max()) and int(xq[2].min()) == -128
        assert float(w[2].min()) == -float(w[2].abs().max())
        lo, hi = (p << 4) >> 4, p >> 4
        assert int(torch.minimum(lo[2].min(), hi[2].min())) == -8
        for half in (lo, hi):
            assert sorted(set(half.flatten().tolist())) == list(range(-8, 8))


def test_config_fields_defaults_and_alias():
    assert int8_dynamic_activation_int4_weight is CONFIG
    assert [f.name for f in dataclasses.fields(CONFIG)] == [
        "group_size", "layout", "mapping_type", "act_mapping_type", "set_inductor_config"]
    c = CONFIG()
    assert c.group_size == 32 and c.layout == PlainLayout() and c.mapping_type is SYMM
    assert c.act_mapping_type is MappingType.ASYMMETRIC and c.set_inductor_config is True
    assert CutlassInt4PackedLayout() == CutlassInt4PackedLayout()


@pytest.mark.parametrize("case", ["plain_default", "tiled_layout", "asym_act", "asym_weight",
                                  "k_not_32", "fp32_weight", "second_module"])
def test_refusals_leave_modules_untouched_and_name_the_served_spelling(case):
    K = 48 if case == "k_not_32" else 64
    dtype = torch.float32 if case == "fp32_weight" else torch.bfloat16
    good = torch.nn.Linear(64, 32, dtype=torch.bfloat16)
    bad = torch.nn.Linear(K, 32, dtype=dtype)
    config = {
        "plain_default": CONFIG(),
        "tiled_layout": CONFIG(layout=TensorCoreTiledLayout(), act_mapping_type=SYMM),
        "asym_act": CONFIG(layout=CutlassInt4PackedLayout()),
        "asym_weight": served(mapping_type=MappingType.ASYMMETRIC),
        # group_size 16 divides 48, so the linear is not skipped and K % 32 decides
        "k_not_32": served(group_size=16),
        "fp32_weight": served(),
        "second_module": served(group_size=16),
    }[case]
    if case == "second_module":  # the refusal comes from a later module: the first stays too
        bad = torch.nn.Linear(48, 32, dtype=torch.bfloat16)
    model = torch.nn.Sequential(good, bad)
    before = [m.weight for m in model]
    with pytest.raises(NotImplementedError, match=r"layout=CutlassInt4PackedLayout\(\)") as e:
        quantize_(model, config)
    assert "Int8DynamicActivationInt4WeightConfig(" in str(e.value)
    assert "MappingType.SYMMETRIC" in str(e.value)
    for m, w in zip(model, before):
        assert m.weight is w and type(m.weight) is torch.nn.Parameter


def test_group_size_only_decides_the_skip():
    rec = load_golden(FIXTURES[1])  # K = 256
    skipped = _linear(rec)
    w0 = skipped.weight
    quantize_(skipped, served(group_size=96))  # 256 % 96 != 0
    assert skipped.weight is w0
    a, b, c = _linear(rec), _linear(rec), _linear(rec)
    quantize_(a, served(group_size=32))
    quantize_(b, served(group_size=128))
    quantize_(c, served(group_size=-1))
    ia, ib, ic = (m.weight.original_weight_tensor.tensor_impl for m in (a, b, c))
    assert torch.equal(ia.int_data, ib.int_data) and torch.equal(ia.scale, ib.scale)
    assert torch.equal(ia.int_data, ic.int_data) and tuple(ia.scale.shape) == (64,)


@pytest.mark.parametrize("fname", FIXTURES)
def test_quantized_structure_and_bytes_match_reference(fname):
    rec = load_golden(fname)
    N, K = int(rec["N"]), int(rec["K"])
    lin = _linear(rec)
    quantize_(lin, served())
    wt = lin.weight
    assert isinstance(wt, LinearActivationQuantizedTensor)
    assert wt.input_quant_func is _int8_symm_cutlass_quant and wt.quant_kwargs == {}
    aqt = wt.original_weight_tensor
    assert isinstance(aqt, AffineQuantizedTensor) and aqt.dtype == torch.bfloat16
    assert tuple(aqt.shape) == (N, K) and tuple(aqt.block_size) == (1, K)
    assert (aqt.quant_min, aqt.quant_max) == (-8, 7)
    assert aqt.zero_point_domain == ZeroPointDomain.NONE
    impl = aqt.tensor_impl
    assert isinstance(impl, Int4PackedTensorImpl) and impl.get_layout() == CutlassInt4PackedLayout()
    assert impl.__tensor_flatten__() == (["int_data", "scale"], [CutlassInt4PackedLayout()])
    assert impl.int_data.dtype == torch.int8 and tuple(impl.int_data.shape) == (N, K // 2)
    assert impl.scale.dtype == torch.float32 and tuple(impl.scale.shape) == (N,)
    assert torch.equal(impl.int_data, torch.from_numpy(rec["wq_packed"]))
    assert torch.equal(impl.scale, torch.from_numpy(rec["ws"]))
    # the weight quantizer on its own, and get_plain / from_plain both ways
    again = _int4_symm_cutlass_quant(bf16(rec["w"])).tensor_impl
    assert torch.equal(again.int_data, impl.int_data) and torch.equal(again.scale, impl.scale)
    q, s, z = impl.get_plain()
    assert z is None and q.dtype == torch.int8 and tuple(q.shape) == (N, K)
    assert int(q.min()) == -8 and int(q.max()) == 7
    p = torch.from_numpy(rec["wq_packed"])
    assert torch.equal(q[:, 0::2], (p << 4) >> 4) and torch.equal(q[:, 1::2], p >> 4)
    back = Int4PackedTensorImpl.from_plain(q, s, None, CutlassInt4PackedLayout())
    assert torch.equal(back.int_data, impl.int_data)
    assert torch.equal(back.get_plain()[0], q)
    # detach and copy_
    d = impl.detach()
    assert isinstance(d, Int4PackedTensorImpl) and torch.equal(d.int_data, impl.int_data)
    dst = Int4PackedTensorImpl(torch.zeros_like(impl.int_data), torch.zeros_like(impl.scale),
                               CutlassInt4PackedLayout())
    dst.copy_(impl)
    assert torch.equal(dst.int_data, impl.int_data) and torch.equal(dst.scale, impl.scale)
    with pytest.raises(ValueError, match="metadata"):
        dst.copy_(Int4PackedTensorImpl(impl.int_data[:8], impl.scale[:8], CutlassInt4PackedLayout()))


@pytest.mark.parametrize("fname", FIXTURES)
def test_activation_quantizer_matches_reference(fname):
    rec = load_golden(fname)
    x = bf16(rec["x"])
    qx = _int8_symm_cutlass_quant(x)
    assert isinstance(qx, AffineQuantizedTensor) and isinstance(qx._layout, PlainLayout)
    assert qx.zero_point_domain == ZeroPointDomain.NONE and qx.tensor_impl.zero_point is None
    assert (qx.quant_min, qx.quant_max) == (None, None)
    assert qx.tensor_impl.scale.dtype == torch.float32
    assert torch.equal(qx.tensor_impl.int_data, torch.from_numpy(rec["xq"]))
    assert torch.equal(qx.tensor_impl.scale, torch.from_numpy(rec["xs"]))
    assert float(qx.tensor_impl.scale[1]) == 2.0 ** -23  # the zero token: eps
    x3 = x.reshape(2, 3, -1)
    q3 = _int8_symm_cutlass_quant(x3)
    assert tuple(q3.tensor_impl.scale.shape) == (2, 3)
    assert torch.equal(q3.tensor_impl.int_data.reshape(6, -1), torch.from_numpy(rec["xq"]))


@pytest.mark.parametrize("fname", FIXTURES)
def test_cpu_forward_equals_y_ref(fname):
    rec = load_golden(fname)
    lin = _linear(rec)
    quantize_(lin, served())
    x = bf16(rec["x"])
    y_ref = bf16(rec["y_ref"])
    y = lin(x)
    assert y.dtype == torch.bfloat16 and torch.equal(y, y_ref)
    for m in (1, 2):  # the zero token gives exactly bf16(bias), or 0 without one
        assert torch.equal(lin(x[m:m + 1]), y_ref[m:m + 1])
    want = bf16(rec["bias"]) if "bias" in rec.files else torch.zeros(int(rec["N"]))
    assert torch.equal(y[1].float(), want.float())
    assert torch.equal(lin(x.reshape(2, 3, -1)), y_ref.reshape(2, 3, -1))


def test_dispatch_table_entry():
    from torchao.dtypes import affine_quantized_tensor_ops as ops_mod
    from torchao.dtypes.uintx.cutlass_int4_packed_layout import (
        _linear_int8_act_int4_weight_cutlass_check,
        _linear_int8_act_int4_weight_cutlass_impl,
    )

    table = ops_mod._AQT_QLINEAR_DISPATCH_TABLE
    assert (table[_linear_int8_act_int4_weight_cutlass_check]
            is _linear_int8_act_int4_weight_cutlass_impl)
    rec = load_golden(FIXTURES[1])
    lin = _linear(rec)
    quantize_(lin, served())
    w = lin.weight.original_weight_tensor
    x = bf16(rec["x"])
    qx = _int8_symm_cutlass_quant(x)
    assert _linear_int8_act_int4_weight_cutlass_check(qx, w, lin.bias)
    first = next(c for c in table if c(qx, w, lin.bias))
    assert first is _linear_int8_act_int4_weight_cutlass_check
    assert not _linear_int8_act_int4_weight_cutlass_check(x, w, None)
    assert not _linear_int8_act_int4_weight_cutlass_check(qx, w, lin.bias.float())


def test_reference_checkpoint_loads_weights_only():
    io_rec = load_golden(CKPT + "_io.npz")
    sd = torch.load(os.path.join(GOLDEN, CKPT + ".pt"), weights_only=True)
    assert sorted(sd) == ["0.bias", "0.weight"]
    wt = sd["0.weight"]
    assert isinstance(wt, LinearActivationQuantizedTensor)
    assert wt.input_quant_func is _int8_symm_cutlass_quant
    impl = wt.original_weight_tensor.tensor_impl
    assert isinstance(impl, Int4PackedTensorImpl)
    lin = _linear(io_rec)
    local = _linear(io_rec)
    quantize_(local, served())
    assert torch.equal(impl.int_data, local.weight.original_weight_tensor.tensor_impl.int_data)
    assert torch.equal(impl.scale, local.weight.original_weight_tensor.tensor_impl.scale)
    model = torch.nn.Sequential(lin)
    model.load_state_dict(sd, assign=True)
    x = bf16(io_rec["x"])
    assert torch.equal(model(x), bf16(io_rec["y_ref"]))
    assert torch.equal(local(x), bf16(io_rec["y_ref"]))


def test_native_dispatch_sets():
    assert ops.native_dispatch() == {"int4_weight_only_linear", "int8_weight_only_linear",
                                     "int8_quantize_per_token", "int8_scaled_mm",
                                     "int8_dyn_linear"}, ops._native_error
    assert ops.native_dispatch_w4a8() == {"rowwise_scaled_linear_cutlass_s8s4",
                                          "int8_quantize_per_token_f32",
                                          "int4_quantize_rows_packed", "w4a8_dyn_linear"}
    assert set(_lib.exported_symbols()) >= {
        "tao_int8_quant_per_token_f32", "tao_int4_quantize_rows_packed_bf16",
        "tao_w4a8_scaled_mm_bf16", "tao_w4a8_dyn_linear_bf16"}


def test_meta_kernels_shapes_and_dtypes():
    T = torch.ops.torchao
    with torch.device("meta"):
        xq = torch.empty(2, 3, 64, dtype=torch.int8)
        xs = torch.empty(2, 3, dtype=torch.float32)
        w = torch.empty(40, 32, dtype=torch.int8)
        ws = torch.empty(40, dtype=torch.float32)
        b = torch.empty(40, dtype=torch.bfloat16)
        x = torch.empty(2, 3, 64, dtype=torch.bfloat16)
        y = T.rowwise_scaled_linear_cutlass_s8s4(xq, xs, w, ws, b, torch.bfloat16)
        assert tuple(y.shape) == (2, 3, 40) and y.dtype == torch.bfloat16
        y = ops.rowwise_scaled_linear_cutlass_s8s4(xq, xs, w, ws)
        assert tuple(y.shape) == (2, 3, 40) and y.dtype == torch.bfloat16
        with pytest.raises(RuntimeError, match="bfloat16 output only"):
            T.rowwise_scaled_linear_cutlass_s8s4(xq, xs, w, ws, None, torch.float16)
        with pytest.raises(RuntimeError, match="multiple of 32"):
            T.rowwise_scaled_linear_cutlass_s8s4(xq[..., :48], xs, w[:, :24], ws, None, None)
        q, s = T.int8_quantize_per_token_f32(x)
        assert tuple(q.shape) == (2, 3, 64) and q.dtype == torch.int8
        assert tuple(s.shape) == (2, 3) and s.dtype == torch.float32
        p, s = T.int4_quantize_rows_packed(torch.empty(40, 64, dtype=torch.bfloat16))
        assert tuple(p.shape) == (40, 32) and p.dtype == torch.int8
        assert tuple(s.shape) == (40,) and s.dtype == torch.float32
        y = T.w4a8_dyn_linear(x, w, ws, b)
        assert tuple(y.shape) == (2, 3, 40) and y.dtype == torch.bfloat16


def _call(name, *args):
    lib = _lib.lib()
    rc = getattr(lib, name)(*args)
    return rc, lib.tao_last_error().decode()


def test_c_abi_argument_checks_before_any_device_work():
    p = 16
    rc, msg = _call("tao_w4a8_scaled_mm_bf16", p, p, p, p, None, p, 1, 8, 48, None)
    assert rc == 1 and "multiple of 32" in msg
    rc, msg = _call("tao_w4a8_scaled_mm_bf16", p, p, p, p, None, p, 1, 8, 131072, None)
    assert rc == 1 and "131072" in msg
    rc, msg = _call("tao_w4a8_scaled_mm_bf16", p, p, p, p, None, p, -1, 8, 64, None)
    assert rc == 1 and "negative" in msg
    rc, msg = _call("tao_w4a8_scaled_mm_bf16", 8, p, p, p, None, p, 1, 8, 64, None)
    assert rc == 1 and "aligned" in msg
    rc, msg = _call("tao_w4a8_dyn_linear_bf16", p, p, p, None, p, 2, 8, 64, None)
    assert rc == 1 and "one token" in msg
    rc, msg = _call("tao_w4a8_dyn_linear_bf16", p, p, p, None, p, 1, 8, 65536 + 32, None)
    assert rc == 1 and "65536" in msg
    rc, msg = _call("tao_int8_quant_per_token_f32", p, p, p, 1, 12, None)
    assert rc == 1 and "multiple of 8" in msg
    rc, msg = _call("tao_int4_quantize_rows_packed_bf16", p, p, p, 1, 12, None)
    assert rc == 1 and "multiple of 8" in msg
    for name, args in (("tao_w4a8_scaled_mm_bf16", (p, p, p, p, None, p, 0, 8, 64, None)),
                       ("tao_w4a8_dyn_linear_bf16", (p, p, p, None, p, 0, 8, 64, None)),
                       ("tao_int8_quant_per_token_f32", (p, p, p, 0, 64, None)),
                       ("tao_int4_quantize_rows_packed_bf16", (p, p, p, 0, 64, None))):
        assert _call(name, *args)[0] == 0, name
